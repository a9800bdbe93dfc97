// rh_channels.h -- turbine output channels of batched cases, written once for host and device.
//
// FP64 restatement of the per-rotor channels FOWT.saveTurbineOutputs leaves in case_metrics: the
// nacelle acceleration AxRNA and tower-base bending moment Mbase of FOWT.rotor_channels and
// FOWT._aero_outputs (raft/fowt.py), and, with the control loop closed (aeroServoMod 2), the rotor
// speed, generator torque and blade pitch through the control transfer function C of Rotor.calcAero
// (raft/rotor.py:373-375).  Built on rh_aero.h: the drivetrain denominator, a(w), b(w), the mean load
// and the numpy complex quotient are the ones the aero-servo matrices use.
//
// Like rh_aero.h: the sums in the Python's order, complex products and quotients written out in real
// arithmetic the way numpy forms them, no fused multiply-add, no library call (the sine of the mean
// pitch is taken by the caller).  |x|^2 is re^2 + im^2 where numpy squares hypot(re, im), and Mbase
// of a rotor without aero is formed as _aero_outputs' M_I + M_w where the host multiplies
// rotor_channels' expanded coefficients: a few roundings either way.  Non-finite inputs propagate.
// The same code is compiled for gfx950 (rh_channels.hip) and for the CPU check against the Python
// (tests/test_channels_host.py builds tools/channels_host.cpp with g++).
#pragma once
#include "rh_aero.h"

namespace rh {
namespace chan {

// the per-pair channel row (enum rh_chan_pair_field of rafthip.h) and the per-rotor geometry row
// (enum rh_chan_geom_field); kept in step by a static_assert in rh_channels.hip and
// tools/channels_host.cpp
constexpr int kZhub = 0, kKpTau = 1, kKiTau = 2, kPairCount = 4;
constexpr int kZrel = 0, kMt = 1, kZcg = 2, kHarm = 3, kIcg = 4, kG = 5, kZbase = 6, kHasTower = 7, kGeomCount = 8;
// the channels (enum rh_turbine_channel): five with a spectrum, then the mean power
constexpr int kAxRNA = 0, kMbase = 1, kOmega = 2, kTorque = 3, kBPitch = 4, kSpectra = 5, kPower = 5, kMeans = 6;

constexpr double kRadps2Rpm = 0.1047;          // raft/helpers.py:32, as _aero_outputs divides by it
constexpr double kRad2Deg = 57.29577951308232;
constexpr double kGravityAx = 9.81;            // raft/raft_fowt.py:1914

// (ar + i ai) (br + i bi) as numpy's complex product forms it
RH_HD inline void cmul(double ar, double ai, double br, double bi, double& cr, double& ci) {
  RH_AERO_NOFMA
  cr = ar * br - ai * bi;
  ci = ar * bi + ai * br;
}

// The control transfer function C(w) = i w (dQ/dU - k_float dQ/dpitch / z_hub) / D(w) of a mode-2 pair
RH_HD inline void control_tf(const double* par, const aero::Derivs& d, double z_hub, double w, double& re, double& im) {
  RH_AERO_NOFMA
  const double s = d.dQ_dU - par[aero::kKfloat] * d.dQ_dPi / z_hub;
  double den_re, den_im;
  aero::denominator(par, d, w, den_re, den_im);
  aero::cdiv(0.0 * s, w * s, den_re, den_im, re, im);
}

// Everything of one (case, rotor) that does not depend on the bin.  mode: 0 without a pair, else the
// pair's aeroServoMod.
struct Rotor {
  double z_rel, m_t, zCG, hArm, I_CG, g, lever2;
  bool tower;
  int mode;
  const double* par;     // the pair's rh_rotor_aero_mb parameter row (mode != 0)
  aero::Derivs d;
  double P00, z_hub, kp_tau, ki_tau;
};

RH_HD inline Rotor rotor_of(const double* geom, const double* par, const double* dloads6, const double* pair_row) {
  RH_AERO_NOFMA
  Rotor r;
  r.z_rel = geom[kZrel], r.m_t = geom[kMt], r.zCG = geom[kZcg], r.hArm = geom[kHarm], r.I_CG = geom[kIcg];
  r.g = geom[kG];
  const double arm = geom[kZrel] - geom[kZbase];
  r.lever2 = arm * arm;
  r.tower = geom[kHasTower] != 0.0;
  r.par = par;
  r.mode = 0;
  r.P00 = 0.0, r.z_hub = 1.0, r.kp_tau = 0.0, r.ki_tau = 0.0;
  r.d = aero::Derivs{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (par) {
    r.mode = par[aero::kMode] == 2.0 ? 2 : 1;
    r.d = aero::load_derivs(dloads6);
    r.P00 = par[aero::kRq] * par[aero::kRq];     // aero::pattern's entry (0, 0): q[0] q[0], q = R_q[:, 0]
    r.z_hub = pair_row[kZhub], r.kp_tau = pair_row[kKpTau], r.ki_tau = pair_row[kKiTau];
  }
  return r;
}

// ... and of one bin of it
struct Bin {
  double w, w2, tx_re, tx_im, c_re, c_im;   // tx: -(-w^2 A00 + i w B00) (z_rel - zBase)^2
};

RH_HD inline Bin bin_of(const Rotor& r, double w) {
  RH_AERO_NOFMA
  Bin b;
  b.w = w, b.w2 = w * w;
  b.tx_re = 0.0, b.tx_im = 0.0, b.c_re = 0.0, b.c_im = 0.0;
  if (r.mode != 0) {
    double a, bb;
    aero::bin_coefficients(r.par, r.d, w, a, bb);
    const double A00 = a * r.P00, B00 = bb * r.P00;
    b.tx_re = -(-b.w2 * A00 + 0.0 * B00) * r.lever2;
    b.tx_im = -(w * B00) * r.lever2;
    if (r.mode == 2) control_tf(r.par, r.d, r.z_hub, w, b.c_re, b.c_im);
  }
  return b;
}

// (i w kp + ki) phi
RH_HD inline void pi_response(double w, double kp, double ki, double p_re, double p_im, double& re, double& im) {
  RH_AERO_NOFMA
  cmul(0.0 * kp + ki, w * kp, p_re, p_im, re, im);
}

RH_HD inline double abs2(double re, double im) {
  RH_AERO_NOFMA
  return re * re + im * im;
}

// |x|^2 of the three control channels from phi (before the unit factors)
RH_HD inline void control_abs2(const Rotor& r, const Bin& b, double p_re, double p_im, double* m2) {
  double x_re, x_im;
  cmul(0.0, b.w, p_re, p_im, x_re, x_im);
  m2[kOmega] = abs2(x_re, x_im);
  pi_response(b.w, r.kp_tau, r.ki_tau, p_re, p_im, x_re, x_im);
  m2[kTorque] = abs2(x_re, x_im);
  pi_response(b.w, r.par[aero::kKpBeta], r.par[aero::kKiBeta], p_re, p_im, x_re, x_im);
  m2[kBPitch] = abs2(x_re, x_im);
}

// |x|^2 [5] of one response row at one bin from its surge and pitch amplitudes
RH_HD inline void row_abs2(const Rotor& r, const Bin& b, double s_re, double s_im, double p_re, double p_im, double* m2) {
  RH_AERO_NOFMA
  const double h_re = s_re + r.z_rel * p_re, h_im = s_im + r.z_rel * p_im;     // XiHub
  m2[kAxRNA] = abs2(b.w2 * h_re, b.w2 * h_im);
  m2[kMbase] = 0.0, m2[kOmega] = 0.0, m2[kTorque] = 0.0, m2[kBPitch] = 0.0;
  if (r.tower) {
    const double a_re = -b.w2 * (s_re + r.zCG * p_re), a_im = -b.w2 * (s_im + r.zCG * p_im);     // aCG
    const double mi_re = -r.m_t * a_re * r.hArm - r.I_CG * (-b.w2 * p_re);
    const double mi_im = -r.m_t * a_im * r.hArm - r.I_CG * (-b.w2 * p_im);
    const double mw = r.m_t * r.g * r.hArm;
    double x_re = mi_re + mw * p_re, x_im = mi_im + mw * p_im;
    if (r.mode != 0) {
      double mx_re, mx_im;
      cmul(b.tx_re, b.tx_im, p_re, p_im, mx_re, mx_im);
      x_re = (x_re + 0.0) + mx_re, x_im = x_im + mx_im;
    }
    m2[kMbase] = abs2(x_re, x_im);
  }
  if (r.mode == 2) {
    double f_re, f_im;
    cmul(b.c_re, b.c_im, h_re, h_im, f_re, f_im);
    control_abs2(r, b, f_re, f_im, m2);
  }
}

// ... and of the wind row of a mode-2 pair, whose motion is zero: phi = C (0 - V_w / (i w)).  m2 [5],
// the two motion channels zero.
RH_HD inline void wind_abs2(const Rotor& r, const Bin& b, double vw, double* m2) {
  RH_AERO_NOFMA
  double q_re, q_im, f_re, f_im;
  aero::cdiv(vw, 0.0, 0.0, b.w, q_re, q_im);
  cmul(b.c_re, b.c_im, 0.0 - q_re, 0.0 - q_im, f_re, f_im);
  m2[kAxRNA] = 0.0, m2[kMbase] = 0.0;
  control_abs2(r, b, f_re, f_im, m2);
}

// getPSD's term of one row, and the channel's unit factor on the summed PSD and on the RMS
RH_HD inline double psd_term(double m2, double dw) {
  RH_AERO_NOFMA
  return 0.5 * m2 / dw;
}

RH_HD inline double psd_units(int ch, double p) {
  RH_AERO_NOFMA
  if (ch == kOmega) {
    const double rpm1 = 1.0 / kRadps2Rpm;
    return rpm1 * rpm1 * p;
  }
  if (ch == kBPitch) return kRad2Deg * kRad2Deg * p;
  return p;
}

RH_HD inline double rms_units(int ch, double rms) {
  RH_AERO_NOFMA
  if (ch == kOmega) return rms / kRadps2Rpm;
  if (ch == kBPitch) return rms * kRad2Deg;
  return rms;
}

// The six means of one (case, rotor).  sin_pitch0: the sine of the case's mean pitch; loads8 and op5
// the pair's rows of rh_rotor_loads (mode != 0).
RH_HD inline void means(const Rotor& r, double sin_pitch0, const double* loads8, const double* op5, double* avg) {
  RH_AERO_NOFMA
  for (int k = 0; k < kMeans; ++k) avg[k] = 0.0;
  avg[kAxRNA] = fabs(sin_pitch0 * kGravityAx);
  if (r.tower) {
    avg[kMbase] = r.m_t * r.g * r.hArm * sin_pitch0;
    if (r.mode != 0) {
      double f6[6];
      aero::mean_load(r.par, loads8, f6);
      // transform_force(f6, [0, 0, -hArm])[4]: np.cross's second entry, offset_z f_x - offset_x f_z
      avg[kMbase] += f6[4] + ((-r.hArm) * f6[0] - 0.0 * f6[2]);
    }
  }
  if (r.mode == 2) {
    avg[kOmega] = op5[1];
    avg[kTorque] = loads8[3] / r.par[aero::kNg];
    avg[kBPitch] = op5[2];
    avg[kPower] = loads8[7];
  }
}

// The pair of case rows [first, past) that names rotor ir: its index, or -1.  max_pairs bounds the
// loop; every index read lies in [first, past).
RH_HD inline int pair_of_rotor(const int* pair_rotor, int first, int past, int max_pairs, int ir) {
  int hit = -1;
  for (int k = 0; k < max_pairs; ++k)
    if (first + k < past && pair_rotor[first + k] == ir) hit = first + k;
  return hit;
}

// What the entry refuses in the host pair columns: 0 if they are fine, else the reason, with the pair
// in *where.
enum Refusal { kFine = 0, kCaseRange, kCaseDecreases, kTooManyPairs, kMode, kRotorRange, kRotorTwice, kVwRange };

inline int check_pairs(int ncase, int nrot, int npair, int nvw, int max_pairs, const int* pair_case, const int* pair_rotor,
                       const int* pair_mode, const int* pair_vw, int* where) {
  int run = 0;
  for (int p = 0; p < npair; ++p) {
    *where = p;
    const int c = pair_case[p];
    if (c < 0 || c >= ncase) return kCaseRange;
    if (p > 0 && c < pair_case[p - 1]) return kCaseDecreases;
    run = (p > 0 && c == pair_case[p - 1]) ? run + 1 : 1;
    if (run > max_pairs) return kTooManyPairs;
  }
  for (int p = 0; p < npair; ++p) {     // (a case's run is at most max_pairs long from here on)
    *where = p;
    run = (p > 0 && pair_case[p] == pair_case[p - 1]) ? run + 1 : 1;
    if (pair_mode[p] != 1 && pair_mode[p] != 2) return kMode;
    if (pair_rotor[p] < 0 || pair_rotor[p] >= nrot) return kRotorRange;
    for (int q = p - run + 1; q < p; ++q)
      if (pair_rotor[q] == pair_rotor[p]) return kRotorTwice;
    if (pair_vw[p] < 0 || pair_vw[p] >= nvw) return kVwRange;
  }
  return kFine;
}

}  // namespace chan
}  // namespace rh
