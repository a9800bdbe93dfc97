// rh_pose.h -- a FOWT's strip-node and member tables at an offset pose, and its mean current
// loads, written once for host and device.
//
// FP64 restatement of Member.setPosition (raft/member.py: the rigid transform of a member's end
// points and unit vectors, the node positions along it), of the pose-dependent columns of
// prep.node_table (raft/prep.py) and of FOWT.calcCurrentLoads (raft/fowt.py).  The same code is
// compiled for gfx950 (rh_pose.hip) and for the CPU check against the Python (tests/test_pose_host.py
// builds tools/pose_host.cpp with g++).  No fused multiply-add: the Python's roundings.
//
// Everything that does not change with the pose (areas, drag coefficients, Imat, a_i, the axial
// coordinate) is a column of the record's node table and is copied, never recomputed.
//
// Every array index below is a compile-time constant once the loops are unrolled (no
// lane-dependent register indexing).
#pragma once
#include <math.h>

#ifndef RH_HD
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif
#endif

#if defined(__clang__)
#define RH_POSE_UNROLL _Pragma("unroll")
#define RH_POSE_NOFMA _Pragma("clang fp contract(off)")
#else
#define RH_POSE_UNROLL
#define RH_POSE_NOFMA
#endif

namespace rh {
namespace pose {

// rows of the record's member table [kMembFields][nmemb] (enum rh_pose_member_field)
enum { kRA0 = 0, kRB0 = 3, kLen = 6, kQ0 = 7, kP10 = 10, kP20 = 13, kMembFields = 16 };

// a member's frame at a pose
struct Frame {
  double rA[3], rB[3], q[3], p1[3], p2[3];
};

// rotation_matrix(X[3], X[4], X[5]) of raft/hydro_math.py (z-y-x intrinsic), row-major
RH_HD inline void rotation(const double* X, double* R) {
  RH_POSE_NOFMA
  const double s1 = sin(X[5]), c1 = cos(X[5]);
  const double s2 = sin(X[4]), c2 = cos(X[4]);
  const double s3 = sin(X[3]), c3 = cos(X[3]);
  R[0] = c1 * c2, R[1] = c1 * s2 * s3 - c3 * s1, R[2] = s1 * s3 + c1 * c3 * s2;
  R[3] = c2 * s1, R[4] = c1 * c3 + s1 * s2 * s3, R[5] = c3 * s1 * s2 - c1 * s3;
  R[6] = -s2, R[7] = c2 * s3, R[8] = c2 * c3;
}

// out = R v
RH_HD inline void rotate(const double* R, double vx, double vy, double vz, double* out) {
  RH_POSE_NOFMA
  out[0] = R[0] * vx + R[1] * vy + R[2] * vz;
  out[1] = R[3] * vx + R[4] * vy + R[5] * vz;
  out[2] = R[6] * vx + R[7] * vy + R[8] * vz;
}

// Member.setPosition: member m of the table mt [kMembFields][nm] at the pose (X[:3], R)
RH_HD inline void member_frame(const double* mt, int nm, int m, const double* X, const double* R, Frame& f) {
  RH_POSE_NOFMA
  rotate(R, mt[(kRA0 + 0) * nm + m], mt[(kRA0 + 1) * nm + m], mt[(kRA0 + 2) * nm + m], f.rA);
  rotate(R, mt[(kRB0 + 0) * nm + m], mt[(kRB0 + 1) * nm + m], mt[(kRB0 + 2) * nm + m], f.rB);
  RH_POSE_UNROLL
  for (int i = 0; i < 3; ++i) {
    f.rA[i] = X[i] + f.rA[i];
    f.rB[i] = X[i] + f.rB[i];
  }
  rotate(R, mt[(kQ0 + 0) * nm + m], mt[(kQ0 + 1) * nm + m], mt[(kQ0 + 2) * nm + m], f.q);
  rotate(R, mt[(kP10 + 0) * nm + m], mt[(kP10 + 1) * nm + m], mt[(kP10 + 2) * nm + m], f.p1);
  rotate(R, mt[(kP20 + 0) * nm + m], mt[(kP20 + 1) * nm + m], mt[(kP20 + 2) * nm + m], f.p2);
}

// component i of r = rA + (ls / l) (rB - rA)
RH_HD inline double node_coord(double rA, double rB, double ls, double l) {
  RH_POSE_NOFMA
  return rA + (ls / l) * (rB - rA);
}

// the member-table column of prep.node_table: [v ; (rA - X[:3]) x v] for q, p1, p2, then |q|^2, |p1|^2, |p2|^2
RH_HD inline double member_six(double ax, double ay, double az, const double* v, double* six) {
  RH_POSE_NOFMA
  six[0] = v[0], six[1] = v[1], six[2] = v[2];
  six[3] = ay * v[2] - az * v[1];
  six[4] = az * v[0] - ax * v[2];
  six[5] = ax * v[1] - ay * v[0];
  return v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
}

RH_HD inline void member_column(const Frame& f, const double* X, double* col) {
  RH_POSE_NOFMA
  const double ax = f.rA[0] - X[0], ay = f.rA[1] - X[1], az = f.rA[2] - X[2];
  col[18] = member_six(ax, ay, az, f.q, col);
  col[19] = member_six(ax, ay, az, f.p1, col + 6);
  col[20] = member_six(ax, ay, az, f.p2, col + 12);
}

// One strip node's current drag (FOWT.calcCurrentLoads): the force f and its moment about X_ref[:3].
// r: node position; q, p1, p2: its member's unit vectors; a*, cd*: the node's drag areas and
// coefficients; vx, vy: the current velocity per unit profile (speed cos, speed sin).
RH_HD inline void current_node_load(const double* r, const double* Xref, const double* q, const double* p1,
                                    const double* p2, double aq, double ap1, double ap2, double aend, double cdq,
                                    double cdp1, double cdp2, double cdend, bool circ, double speed, double ch, double sh,
                                    double depth, double Zref, double shearExp, double rho, double* D) {
  RH_POSE_NOFMA
  const double v = speed * pow((depth - fabs(r[2])) / (depth + Zref), shearExp);
  const double vrel[3] = {v * ch, v * sh, 0.0};
  const double dq = vrel[0] * q[0] + vrel[1] * q[1] + vrel[2] * q[2];
  const double d1 = vrel[0] * p1[0] + vrel[1] * p1[1] + vrel[2] * p1[2];
  const double d2 = vrel[0] * p2[0] + vrel[1] * p2[1] + vrel[2] * p2[2];
  double vq[3], vp[3], vp1[3], vp2[3];
  RH_POSE_UNROLL
  for (int i = 0; i < 3; ++i) {
    vq[i] = dq * q[i];
    vp[i] = vrel[i] - vq[i];
    vp1[i] = d1 * p1[i];
    vp2[i] = d2 * p2[i];
  }
  const double nq = sqrt(vq[0] * vq[0] + vq[1] * vq[1] + vq[2] * vq[2]);
  const double np = sqrt(vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2]);
  const double n1 = circ ? np : sqrt(vp1[0] * vp1[0] + vp1[1] * vp1[1] + vp1[2] * vp1[2]);
  const double n2 = circ ? np : sqrt(vp2[0] * vp2[0] + vp2[1] * vp2[1] + vp2[2] * vp2[2]);
  const double kq = 0.5 * rho * aq * cdq * nq;
  const double k1 = 0.5 * rho * ap1 * cdp1 * n1;
  const double k2 = 0.5 * rho * ap2 * cdp2 * n2;
  const double ke = 0.5 * rho * aend * cdend * nq;
  double f[3];
  RH_POSE_UNROLL
  for (int i = 0; i < 3; ++i) f[i] = kq * vq[i] + k1 * vp1[i] + k2 * vp2[i] + ke * vq[i];
  const double x = r[0] - Xref[0], y = r[1] - Xref[1], z = r[2] - Xref[2];
  D[0] = f[0], D[1] = f[1], D[2] = f[2];
  D[3] = y * f[2] - z * f[1];
  D[4] = z * f[0] - x * f[2];
  D[5] = x * f[1] - y * f[0];
}

}  // namespace pose
}  // namespace rh
