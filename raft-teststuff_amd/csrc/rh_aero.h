// rh_aero.h -- aero-servo added mass and damping of an operating rotor, written once for host and
// device.
//
// FP64 restatement of the bin-dependent part of raft/rotor.py's Rotor.calcAero (aeroServoMod 1 and
// 2, without the wind excitation and the Kaimal spectrum, which the response solve does not read)
// and of the part of FOWT.calcTurbineConstants that moves it to the platform reference point.  The
// hub-frame 6 x 6 of either mode is a scalar times q q^T in its upper-left 3 x 3 (q = R_q[:, 0]), so
// moved by translate_matrix_6to6 it is that scalar times a bin-independent pattern P of the pair:
//   A_aero(w) = a(w) P,  B_aero(w) = b(w) P.
// The same code is compiled for gfx950 (rh_aero.hip) and for the CPU check against the Python
// (tests/test_aero_host.py builds tools/aero_host.cpp with g++).
//
// The complex quotients are written out in real arithmetic the way numpy divides complex numbers
// (Smith's method), the sums in the Python's order, and no fused multiply-add is formed, so the two
// differ by a few roundings (the Python scales R diag(a, 0, 0) R^T per bin and then translates it;
// here the pattern is translated once and scaled per bin).  A vanishing denominator gives the
// Python's inf / nan; no input can make an index leave its array.
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
#define RH_AERO_NOFMA _Pragma("clang fp contract(off)")   // the Python's roundings: no fused multiply-add
#else
#define RH_AERO_NOFMA
#endif

namespace rh {
namespace aero {

// the per-pair parameter row (enum rh_aero_param_field of rafthip.h; kept in step by a static_assert
// in rh_aero.hip and tools/aero_host.cpp)
constexpr int kMode = 0;
constexpr int kRq = 1;        // 9, row-major
constexpr int kRhub = 10;     // 3
constexpr int kIdrive = 13, kNg = 14, kKfloat = 15, kKpBeta = 16, kKiBeta = 17, kKpTau = 18, kKiTau = 19;
constexpr int kGyro = 20;     // 3
constexpr int kParamCount = 24;

constexpr double kRad2Deg = 57.2958;     // raft/rotor.py's RAD2DEG and RPM2RADPS, as rounded there
constexpr double kRpm2Radps = 0.1047;

// (ar + i ai) / (br + i bi) as numpy's complex division forms it
RH_HD inline void cdiv(double ar, double ai, double br, double bi, double& cr, double& ci) {
  RH_AERO_NOFMA
  const double br_abs = fabs(br), bi_abs = fabs(bi);
  if (br_abs >= bi_abs) {
    if (br_abs == 0.0 && bi_abs == 0.0) {
      cr = ar / br_abs;
      ci = ai / bi_abs;
      return;
    }
    const double rat = bi / br;
    const double scl = 1.0 / (br + bi * rat);
    cr = (ar + ai * rat) * scl;
    ci = (ai - ar * rat) * scl;
  } else {
    const double rat = br / bi;
    const double scl = 1.0 / (bi + br * rat);
    cr = (ar * rat + ai) * scl;
    ci = (ai * rat - ar) * scl;
  }
}

// The six derivatives of rh_rotor_loads, d(T, Q)/d(Uinf, Omega [rpm], pitch [deg]), in calcAero's units
struct Derivs {
  double dT_dU, dT_dOm, dT_dPi, dQ_dU, dQ_dOm, dQ_dPi;
};

RH_HD inline Derivs load_derivs(const double* d6) {
  RH_AERO_NOFMA
  Derivs d;
  d.dT_dU = d6[0];
  d.dT_dOm = d6[1] / kRpm2Radps;
  d.dT_dPi = d6[2] * kRad2Deg;
  d.dQ_dU = d6[3];
  d.dQ_dOm = d6[4] / kRpm2Radps;
  d.dQ_dPi = d6[5] * kRad2Deg;
  return d;
}

// The real and imaginary parts of the drivetrain denominator of H_QT at w (raft/rotor.py:373-378)
RH_HD inline void denominator(const double* par, const Derivs& d, double w, double& re, double& im) {
  RH_AERO_NOFMA
  const double kp_beta = par[kKpBeta], ki_beta = par[kKiBeta];
  const double c1 = (d.dQ_dOm + kp_beta * d.dQ_dPi) - par[kNg] * par[kKpTau];
  re = ((par[kIdrive] * (w * w) + 0.0) + ki_beta * d.dQ_dPi) - par[kNg] * par[kKiTau];
  im = c1 * w;
}

// a(w) and b(w) of one pair at one bin: the scalars of A_aero = a P and B_aero = b P
RH_HD inline void bin_coefficients(const double* par, const Derivs& d, double w, double& a, double& b) {
  RH_AERO_NOFMA
  if (par[kMode] != 2.0) {   // aeroServoMod 1: the thrust-speed derivative only
    a = 0.0;
    b = d.dT_dU;
    return;
  }
  const double kp_beta = par[kKpBeta], ki_beta = par[kKiBeta], k_float = par[kKfloat];
  double den_re, den_im;
  denominator(par, d, w, den_re, den_im);
  const double num_re = ki_beta * d.dT_dPi;
  const double num_im = (d.dT_dOm + kp_beta * d.dT_dPi) * w;
  double h_re, h_im;
  cdiv(num_re, num_im, den_re, den_im, h_re, h_im);
  const double r1 = d.dT_dU - k_float * d.dT_dPi;
  const double r2 = d.dQ_dU - k_float * d.dQ_dPi;
  const double x_re = r1 - h_re * r2;
  const double x_im = 0.0 - h_im * r2;
  double q_re, q_im;
  cdiv(x_re, x_im, 0.0, w, q_re, q_im);   // X / (i w)
  a = q_re;
  b = x_re;
}

// alternator(r) (getH), row-major 3 x 3
RH_HD inline void alternator(const double* r, double* H) {
  H[0] = 0.0, H[1] = r[2], H[2] = -r[1];
  H[3] = -r[2], H[4] = 0.0, H[5] = r[0];
  H[6] = r[1], H[7] = -r[0], H[8] = 0.0;
}

// P [36] of a pair: translate_matrix_6to6 of the 6 x 6 whose upper-left 3 x 3 is q q^T, q = R_q[:, 0],
// by r_hub_rel
RH_HD inline void pattern(const double* par, double* P) {
  RH_AERO_NOFMA
  const double q[3] = {par[kRq + 0], par[kRq + 3], par[kRq + 6]};
  double H[9], m[9], mh[9], hm[9];
  alternator(par + kRhub, H);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[i * 3 + j] = q[i] * q[j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      mh[i * 3 + j] = (m[i * 3 + 0] * H[0 * 3 + j] + m[i * 3 + 1] * H[1 * 3 + j]) + m[i * 3 + 2] * H[2 * 3 + j];
      hm[i * 3 + j] = (H[i * 3 + 0] * m[0 * 3 + j] + H[i * 3 + 1] * m[1 * 3 + j]) + H[i * 3 + 2] * m[2 * 3 + j];
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      P[i * 6 + j] = m[i * 3 + j];
      P[i * 6 + 3 + j] = mh[i * 3 + j];          // m H
      P[(3 + j) * 6 + i] = mh[i * 3 + j];        // its transpose
      P[(3 + i) * 6 + 3 + j] =                   // (H m) H^T
          (hm[i * 3 + 0] * H[j * 3 + 0] + hm[i * 3 + 1] * H[j * 3 + 1]) + hm[i * 3 + 2] * H[j * 3 + 2];
    }
}

// The pair's mean aero load about the platform reference point:
// transform_force(R_q (T, Y, Z), R_q (My, Q, Mz); r_hub_rel), loads8 = T, Y, Z, Q, My, Mz, Mb, P
RH_HD inline void mean_load(const double* par, const double* loads8, double* f6) {
  RH_AERO_NOFMA
  const double F[3] = {loads8[0], loads8[1], loads8[2]};
  const double Mo[3] = {loads8[4], loads8[3], loads8[5]};
  const double* R = par + kRq;
  const double* r = par + kRhub;
  double f[3], m[3];
  for (int i = 0; i < 3; ++i) {
    f[i] = (R[i * 3 + 0] * F[0] + R[i * 3 + 1] * F[1]) + R[i * 3 + 2] * F[2];
    m[i] = (R[i * 3 + 0] * Mo[0] + R[i * 3 + 1] * Mo[1]) + R[i * 3 + 2] * Mo[2];
  }
  f6[0] = f[0], f6[1] = f[1], f6[2] = f[2];
  f6[3] = m[0] + (r[1] * f[2] - r[2] * f[1]);
  f6[4] = m[1] + (r[2] * f[0] - r[0] * f[2]);
  f6[5] = m[2] + (r[0] * f[1] - r[1] * f[0]);
}

// The gyroscopic damping of a case: alternator of the summed gyroscopic vectors in G36[3:, 3:], zeros
// elsewhere (the Python adds the whole 6 x 6, B_gyro, to every bin's B)
RH_HD inline void gyro_matrix(const double* gsum, double* G36) {
  double H[9];
  alternator(gsum, H);
  for (int k = 0; k < 36; ++k) G36[k] = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) G36[(3 + i) * 6 + 3 + j] = H[i * 3 + j];
}

// One entry of a case's M or B at one bin: the pairs' terms summed in rotor order, then the base
// design's entry (and for B the gyroscopic entry).  coef: the pairs' a or b at this bin, `stride` apart;
// P: the pairs' patterns' entries, 36 apart.  npair = 0 returns the base entry unchanged.
RH_HD inline double entry(int npair, int max_pairs, const double* coef, int stride, const double* P, double base) {
  RH_AERO_NOFMA
  if (npair <= 0) return base;
  double s = coef[0] * P[0];
  for (int k = 1; k < max_pairs; ++k)
    if (k < npair) s += coef[(long)k * stride] * P[k * 36];
  return s + base;
}

// ... and of B: (the pairs' terms + the base entry) + the gyroscopic entry
RH_HD inline double damping_entry(int npair, int max_pairs, const double* coef, int stride, const double* P, double base,
                                  double gyro) {
  RH_AERO_NOFMA
  if (npair <= 0) return base;
  return entry(npair, max_pairs, coef, stride, P, base) + gyro;
}

// The first index of the non-decreasing v [n] whose value is >= key (n if none): the pairs of case
// c are [first_at_least(c), first_at_least(c + 1)).  25 halvings cover n <= 2^24; mid stays in [0, n).
constexpr int kSearchSteps = 25;
RH_HD inline int first_at_least(const int* v, int n, int key) {
  int lo = 0, len = n;
  for (int s = 0; s < kSearchSteps; ++s) {
    if (len > 0) {
      const int half = len >> 1, mid = lo + half;
      if (v[mid] < key) {
        lo = mid + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
  }
  return lo;
}

}  // namespace aero
}  // namespace rh
