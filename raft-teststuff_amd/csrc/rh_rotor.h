// rh_rotor.h -- blade-element momentum rotor loads, written once for host and device.
//
// FP64 restatement, operation for operation, of raft/ccblade.py: the airfoil splines as fitpack's
// bispev evaluates them (fpbisp / fpbspl: clamp to the knot range, find the knot interval, de
// Boor-Cox), wind_components, relative_wind, induction_factors, CCBlade._run_bem (iterRe = 1),
// _loads, _solve_phi with scipy's brentq (xtol 2e-12, rtol 4 eps, 100 iterations), _section_derivs
// and the sector combination of CCBlade.evaluate.  The same code is compiled for gfx950
// (rh_rotor.hip) and for the CPU check against the Python (tests/test_rotor_host.py builds
// tools/rotor_host.cpp with g++).
//
// One call of section_point is one (operating point, sector, section): it is a lane's own work on
// the device.  The sums along the blade (thrust_torque's trapezoids as per-station weights) and
// over the sectors are the caller's: across lanes on the device, section after section on the
// host, so the two agree to rounding, not to the bit.
//
// Lock step: the Brent loop runs until the wave's vote RH_ROTOR_ANY says nobody is left, finished
// and padding lanes predicated off; a lane's result never depends on its neighbours.  On the host
// the vote is the lane's own flag.  Every loop has a fixed upper bound and every table index is
// clamped where it is formed.
#pragma once
#include <math.h>

#ifndef RH_HD
#if defined(__HIPCC__)
#define RH_HD __host__ __device__
#else
#define RH_HD
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define RH_ROTOR_ANY(x) (__any((x)) != 0)
#else
#define RH_ROTOR_ANY(x) (x)
#endif

#if defined(__clang__)
#define RH_ROTOR_UNROLL _Pragma("unroll")
#define RH_ROTOR_NOFMA _Pragma("clang fp contract(off)")   // the Python's roundings: no fused multiply-add
#else
#define RH_ROTOR_UNROLL
#define RH_ROTOR_NOFMA
#endif

namespace rh {
namespace rotor {

// per-point status (0 = fine); a point reports the largest of its sections and its own
enum {
  kOk = 0,
  kNoBracket = 1,   // a section without a sign change in any bracket, or a NaN residual (brentq's ValueError: phi = 0)
  kNonFinite = 2,   // a non-finite load
  kBadRotor = 3     // rot_idx outside [0, nrot)
};

constexpr int kBrentMaxIter = 100;
constexpr int kMaxDegree = 3;
constexpr int kIntervalSteps = 8;          // bisection steps of the knot search: 2^8 > 128 knots
constexpr double kPi = 3.141592653589793;  // numpy.pi
constexpr double kEps = 2.220446049250313e-16;
constexpr double kDeg2Rad = kPi / 180.0;   // numpy.radians multiplies by this constant

RH_HD inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One airfoil polar: RectBivariateSpline.tck / .degrees with degree kx in alpha (nx knots) and
// degree 1 in Re (4 knots, 2 coefficient columns).
struct Spline {
  const double* tx;   // [nx]
  const double* ty;   // [4]
  const double* c;    // [nx - kx - 1][2]
  int nx, kx;
};

// fitpack's fpbspl: the k + 1 non-zero B-splines of degree k at x, t[l] <= x < t[l + 1].  The
// loops are written to their largest extent (kMaxDegree) so that h is indexed by constants.
RH_HD inline void bspl_basis(const double* t, int n, int k, double x, int l, double* h) {
  RH_ROTOR_NOFMA
  double hh[kMaxDegree];
  h[0] = 1.0;
  RH_ROTOR_UNROLL
  for (int j = 1; j <= kMaxDegree; ++j) {
    if (j <= k) {
      RH_ROTOR_UNROLL
      for (int i = 0; i < j; ++i) hh[i] = h[i];
      h[0] = 0.0;
      RH_ROTOR_UNROLL
      for (int i = 1; i <= j; ++i) {
        const double tli = t[clampi(l + i, 0, n - 1)];
        const double tlj = t[clampi(l + i - j, 0, n - 1)];
        if (tli == tlj) {
          h[i] = 0.0;
        } else {
          const double f = hh[i - 1] / (tli - tlj);
          h[i - 1] = h[i - 1] + f * (tli - x);
          h[i] = f * (x - tlj);
        }
      }
    }
  }
}

// fpbisp's knot search: the interval l in [k, n - k - 2] with t[l] <= arg < t[l + 1] (the last one
// at the upper end), as its linear walk finds it on non-decreasing knots.
RH_HD inline int knot_interval(const double* t, int n, int k, double arg) {
  int lo = clampi(k, 0, n - 1), hi = clampi(n - k - 2, lo, n - 1);
  for (int it = 0; it < kIntervalSteps; ++it) {
    if (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (t[mid] <= arg) lo = mid; else hi = mid - 1;
    }
  }
  return lo;
}

// bispev at one point (x = alpha, y = Re)
RH_HD inline double spline_eval(const Spline& s, double x, double y) {
  RH_ROTOR_NOFMA
  const int nx = s.nx, kx = clampi(s.kx, 1, kMaxDegree);
  const double xb = s.tx[clampi(kx, 0, nx - 1)], xe = s.tx[clampi(nx - kx - 1, 0, nx - 1)];
  double ax = x;
  if (ax < xb) ax = xb;
  if (ax > xe) ax = xe;
  const int lx = knot_interval(s.tx, nx, kx, ax);
  double wx[kMaxDegree + 1] = {0.0, 0.0, 0.0, 0.0};
  bspl_basis(s.tx, nx, kx, ax, lx, wx);
  const double yb = s.ty[1], ye = s.ty[2];
  double ay = y;
  if (ay < yb) ay = yb;
  if (ay > ye) ay = ye;
  double wy[kMaxDegree + 1] = {0.0, 0.0, 0.0, 0.0};
  bspl_basis(s.ty, 4, 1, ay, 1, wy);
  const int rows = nx - kx - 1;
  const int row0 = clampi(lx - kx, 0, rows - 1);
  double sp = 0.0;
  RH_ROTOR_UNROLL
  for (int i = 0; i <= kMaxDegree; ++i) {
    if (i <= kx) {
      const int row = clampi(row0 + i, 0, rows - 1);
      sp = sp + s.c[row * 2] * wx[i] * wy[0];
      sp = sp + s.c[row * 2 + 1] * wx[i] * wy[1];
    }
  }
  return sp;
}

struct Blade {
  double Rhub, Rtip, rho, mu, hubHt, shearExp;
  int B;
  bool usecd, tiploss, hubloss, wakerotation;
};

struct Section {
  double r, chord, theta;
  double x_az, y_az, z_az, cone;   // define_curvature of the blade stations
  Spline cl, cd;
};

// Station i of a rotor record's tables (include/rafthip.h, rh_rotor: section [9][nr], nknot [2][nr],
// knots [2][nr][stride + 4], coef [2][nr][stride][2]); i and the knot counts are clamped here.
RH_HD inline Section load_section(const double* section, const int* nknot, const double* knots, const double* coef, int nr,
                                  int kx, int stride, int i, double& weight, double& cone_path) {
  const int ii = clampi(i, 0, nr - 1);
  Section s;
  s.r = section[0 * nr + ii];
  s.chord = section[1 * nr + ii];
  s.theta = section[2 * nr + ii];
  s.x_az = section[3 * nr + ii];
  s.y_az = section[4 * nr + ii];
  s.z_az = section[5 * nr + ii];
  s.cone = section[6 * nr + ii];
  weight = section[7 * nr + ii];
  cone_path = section[8 * nr + ii];
  const int kk = clampi(kx, 1, kMaxDegree);
  for (int p = 0; p < 2; ++p) {
    Spline& sp = p == 0 ? s.cl : s.cd;
    const long row = (long)p * nr + ii;
    sp.nx = clampi(nknot[row], 2 * (kk + 1), stride);
    sp.kx = kk;
    sp.tx = knots + row * (stride + 4);
    sp.ty = sp.tx + stride;
    sp.c = coef + row * stride * 2;
  }
  return s;
}

// wind_components of one section at one azimuth [rad]
RH_HD inline void wind_components(const Blade& b, const Section& s, double yaw, double tilt, double azimuth, double Uinf,
                                  double OmegaRPM, double& Vx, double& Vy) {
  RH_ROTOR_NOFMA
  const double sy = sin(yaw), cy = cos(yaw);
  const double st = sin(tilt), ct = cos(tilt);
  const double sa = sin(azimuth), ca = cos(azimuth);
  const double Omega = OmegaRPM * kPi / 30.0;
  const double sc = sin(s.cone), cc = cos(s.cone);
  const double heightFromHub = (s.y_az * sa + s.z_az * ca) * ct - s.x_az * st;
  const double V = Uinf * pow(1.0 + heightFromHub / b.hubHt, b.shearExp);
  const double Vwind_x = V * ((cy * st * ca + sy * sa) * sc + cy * ct * cc);
  const double Vwind_y = V * (cy * st * sa - sy * ca);
  const double Vrot_x = -Omega * s.y_az * sc;
  const double Vrot_y = Omega * s.z_az;
  Vx = Vwind_x + Vrot_x;
  Vy = Vwind_y + Vrot_y;
}

RH_HD inline void relative_wind(double phi, double a, double ap, double Vx, double Vy, double pitch, double chord,
                                double theta, double rho, double mu, double& alpha, double& W, double& Re) {
  RH_ROTOR_NOFMA
  if (fabs(a) > 10) {
    W = Vy * (1 + ap) / cos(phi);
  } else if (fabs(ap) > 10) {
    W = Vx * (1 - a) / sin(phi);
  } else {
    const double u = Vx * (1 - a), v = Vy * (1 + ap);
    W = sqrt(u * u + v * v);
  }
  alpha = phi - (theta + pitch);
  Re = rho * W * chord / mu;
}

// the BEM residual and the induction factors at inflow angle phi
RH_HD inline void induction_factors(double r, double chord, double Rhub, double Rtip, double phi, double cl, double cd,
                                    int B, double Vx, double Vy, bool usecd, bool hubloss, bool tiploss,
                                    bool wakerotation, double& fzero, double& a, double& ap) {
  RH_ROTOR_NOFMA
  const double sigma_p = B / 2.0 / kPi * chord / r;
  const double sphi = sin(phi), cphi = cos(phi);
  double cn, ct;
  if (usecd) {
    cn = cl * cphi + cd * sphi;
    ct = cl * sphi - cd * cphi;
  } else {
    cn = cl * cphi;
    ct = cl * sphi;
  }
  double Ftip = 1.0;
  if (tiploss) {
    const double factortip = B / 2.0 * (Rtip - r) / (r * fabs(sphi));
    Ftip = 2.0 / kPi * acos(exp(-factortip));
  }
  double Fhub = 1.0;
  if (hubloss) {
    const double factorhub = B / 2.0 * (r - Rhub) / (Rhub * fabs(sphi));
    Fhub = 2.0 / kPi * acos(exp(-factorhub));
  }
  const double F = Ftip * Fhub;
  const double k = sigma_p * cn / 4.0 / F / sphi / sphi;
  double kp = sigma_p * ct / 4.0 / F / sphi / cphi;
  if (phi > 0) {   // momentum / empirical region
    if (k <= 2.0 / 3.0) {
      a = k / (1 + k);
    } else {       // Glauert correction (Buhl)
      const double g1 = 2.0 * F * k - (10.0 / 9 - F);
      const double g2 = 2.0 * F * k - (4.0 / 3 - F) * F;
      const double g3 = 2.0 * F * k - (25.0 / 9 - 2 * F);
      if (fabs(g3) < 1e-6) {
        a = 1.0 - 1.0 / 2.0 / sqrt(g2);
      } else {
        a = (g1 - sqrt(g2)) / g3;
      }
    }
  } else {         // propeller brake region
    a = k > 1.0 ? k / (k - 1.0) : 0.0;
  }
  ap = kp / (1.0 - kp);
  if (!wakerotation) {
    ap = 0.0;
    kp = 0.0;
  }
  const double lambda_r = Vy / Vx;
  if (phi > 0) {
    fzero = sphi / (1.0 - a) - cphi / lambda_r * (1.0 - kp);
  } else {
    fzero = sphi * (1.0 - k) - cphi / lambda_r * (1.0 - kp);
  }
}

// CCBlade._run_bem with iterRe = 1: the inductions start at zero
RH_HD inline void run_bem(const Blade& b, const Section& s, double phi, double Vx, double Vy, double pitch, double& fzero,
                          double& a, double& ap) {
  double alpha, W, Re;
  relative_wind(phi, 0.0, 0.0, Vx, Vy, pitch, s.chord, s.theta, b.rho, b.mu, alpha, W, Re);
  const double cl = spline_eval(s.cl, alpha, Re);
  const double cd = spline_eval(s.cd, alpha, Re);
  induction_factors(s.r, s.chord, b.Rhub, b.Rtip, phi, cl, cd, b.B, Vx, Vy, b.usecd, b.hubloss, b.tiploss, b.wakerotation,
                    fzero, a, ap);
}

struct SectionEval {
  double fzero, a, ap, Np, Tp, alpha, cl, cd, W;
};

// The residual (0 when not rotating) and CCBlade._loads at phi, from one _run_bem (the Python
// calls it twice on the same arguments).
RH_HD inline SectionEval eval_section(const Blade& b, const Section& s, double phi, bool rotating, double Vx, double Vy,
                                      double pitch) {
  RH_ROTOR_NOFMA
  SectionEval e;
  const double cphi = cos(phi), sphi = sin(phi);
  e.fzero = 0.0;
  e.a = e.ap = 0.0;
  if (rotating) run_bem(b, s, phi, Vx, Vy, pitch, e.fzero, e.a, e.ap);
  double Re;
  relative_wind(phi, e.a, e.ap, Vx, Vy, pitch, s.chord, s.theta, b.rho, b.mu, e.alpha, e.W, Re);
  e.cl = spline_eval(s.cl, e.alpha, Re);
  e.cd = spline_eval(s.cd, e.alpha, Re);
  const double cn = e.cl * cphi + e.cd * sphi;   // these always contain drag
  const double ct = e.cl * sphi - e.cd * cphi;
  const double q = 0.5 * b.rho * (e.W * e.W);
  e.Np = cn * q * s.chord;
  e.Tp = ct * q * s.chord;
  return e;
}

struct Residual {
  const Blade& b;
  const Section& s;
  double Vx, Vy, pitch;
  RH_HD double operator()(double phi) const {
    double f, a, ap;
    run_bem(b, s, phi, Vx, Vy, pitch, f, a, ap);
    return f;
  }
};

// scipy.optimize.brentq (Zeros/brentq.c) with its defaults, from the already evaluated ends.  A
// NaN residual or no sign change is brentq's ValueError: the caller's phi = 0, `failed` set.
// `run` = false lanes only keep the wave's loop company.
template <class F>
RH_HD inline double brentq(const F& f, double xa, double xb, double fa, double fb, bool run, bool& failed) {
  RH_ROTOR_NOFMA
  const double xtol = 2e-12, rtol = 4 * kEps;
  double xpre = xa, xcur = xb, xblk = 0.0, fpre = fa, fcur = fb, fblk = 0.0, spre = 0.0, scur = 0.0;
  double result = 0.0;
  bool active = run;
  failed = false;
  if (active) {
    if (fpre != fpre || fcur != fcur) {
      failed = true, active = false;
    } else if (fpre == 0) {
      result = xpre, active = false;
    } else if (fcur == 0) {
      result = xcur, active = false;
    } else if ((fpre < 0) == (fcur < 0)) {
      failed = true, active = false;
    }
  }
  for (int i = 0; i < kBrentMaxIter && RH_ROTOR_ANY(active); ++i) {
    if (active) {
      if (fpre != 0 && fcur != 0 && ((fpre < 0) != (fcur < 0))) {
        xblk = xpre;
        fblk = fpre;
        spre = scur = xcur - xpre;
      }
      if (fabs(fblk) < fabs(fcur)) {
        xpre = xcur, xcur = xblk, xblk = xpre;
        fpre = fcur, fcur = fblk, fblk = fpre;
      }
      const double delta = (xtol + rtol * fabs(xcur)) / 2;
      const double sbis = (xblk - xcur) / 2;
      if (fcur == 0 || fabs(sbis) < delta) {
        result = xcur;
        active = false;
      } else {
        if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
          double stry;
          if (xpre == xblk) {   // interpolate
            stry = -fcur * (xcur - xpre) / (fcur - fpre);
          } else {              // extrapolate
            const double dpre = (fpre - fcur) / (xpre - xcur);
            const double dblk = (fblk - fcur) / (xblk - xcur);
            stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
          }
          const double lim = 3 * fabs(sbis) - delta;
          if (2 * fabs(stry) < (fabs(spre) < lim ? fabs(spre) : lim)) {   // good short step
            spre = scur;
            scur = stry;
          } else {
            spre = sbis;
            scur = sbis;
          }
        } else {
          spre = sbis;
          scur = sbis;
        }
        xpre = xcur;
        fpre = fcur;
        if (fabs(scur) > delta) {
          xcur += scur;
        } else {
          xcur += (sbis > 0 ? delta : -delta);
        }
        fcur = f(xcur);
        if (fcur != fcur) {
          failed = true, active = false;
          result = 0.0;
        }
      }
    }
  }
  if (active) result = xcur;   // 100 iterations: brentq's last iterate (the host raises there)
  return result;
}

// CCBlade._solve_phi: the bracket (1e-6, pi/2], else [-pi/4, -1e-6), else [pi/2, pi - 1e-6).
// bracket: 0 none (not rotating), 1, 2, 3.
RH_HD inline double solve_phi(const Blade& b, const Section& s, bool rotating, double Vx, double Vy, double pitch, bool run,
                              bool& failed, int& bracket) {
  RH_ROTOR_NOFMA
  failed = false;
  bracket = 0;
  const bool solve = run && rotating;
  const Residual f{b, s, Vx, Vy, pitch};
  const double eps = 1e-6;
  double lo = eps, hi = kPi / 2, flo = 1.0, fhi = -1.0;
  if (solve) {
    bracket = 1;
    flo = f(lo);
    fhi = f(hi);
    if (flo * fhi > 0) {   // an uncommon but possible case
      const double f1 = f(-kPi / 4), f2 = f(-eps);
      if (f1 < 0 && f2 > 0) {
        lo = -kPi / 4, hi = -eps, flo = f1, fhi = f2;
        bracket = 2;
      } else {
        lo = kPi / 2, hi = kPi - eps, flo = fhi;
        fhi = f(hi);
        bracket = 3;
      }
    }
  }
  const double root = brentq(f, lo, hi, flo, fhi, solve, failed);
  if (!rotating) return kPi / 2.0;
  return failed ? 0.0 : root;
}

struct PointOut {
  double phi, Np, Tp;
  double dN[3], dT[3];   // d(Np, Tp)/d(Uinf, Omega_rpm, pitch_deg)
  int status, bracket;
};

// (residual, Np, Tp) of CCBlade._section_derivs' f_and_loads
RH_HD inline void f_and_loads(const Blade& b, const Section& s, double phi, bool rotating, double yaw, double tilt,
                              double azimuth, double U, double Om, double pit_deg, double* g) {
  RH_ROTOR_NOFMA
  double Vx, Vy;
  wind_components(b, s, yaw, tilt, azimuth, U, Om, Vx, Vy);
  const SectionEval e = eval_section(b, s, phi, rotating, Vx, Vy, pit_deg * kDeg2Rad);
  g[0] = e.fzero, g[1] = e.Np, g[2] = e.Tp;
}

// One (operating point, sector, section): inflow, root, loads and, with derivs, _section_derivs.
RH_HD inline void section_point(const Blade& b, const Section& s, double Uinf, double Omega, double pitch_deg, double tilt,
                                double yaw, double azimuth, bool derivs, bool run, PointOut& o) {
  RH_ROTOR_NOFMA
  const bool rotating = Omega != 0;
  const double pitch = pitch_deg * kDeg2Rad;
  double Vx, Vy;
  wind_components(b, s, yaw, tilt, azimuth, Uinf, Omega, Vx, Vy);
  bool failed;
  o.phi = solve_phi(b, s, rotating, Vx, Vy, pitch, run, failed, o.bracket);
  o.status = failed ? (int)kNoBracket : (int)kOk;
  o.Np = o.Tp = 0.0;
  RH_ROTOR_UNROLL
  for (int k = 0; k < 3; ++k) o.dN[k] = o.dT[k] = 0.0;
  if (!run) return;
  const SectionEval e = eval_section(b, s, o.phi, rotating, Vx, Vy, pitch);
  o.Np = e.Np;
  o.Tp = e.Tp;
  if (!derivs) return;
  const double phi = o.phi;
  const double hphi = 1e-7 * (fabs(phi) > 1.0 ? fabs(phi) : 1.0);
  double gp[3], gm[3], g_phi[3];
  f_and_loads(b, s, phi + hphi, rotating, yaw, tilt, azimuth, Uinf, Omega, pitch_deg, gp);
  f_and_loads(b, s, phi - hphi, rotating, yaw, tilt, azimuth, Uinf, Omega, pitch_deg, gm);
  RH_ROTOR_UNROLL
  for (int i = 0; i < 3; ++i) g_phi[i] = (gp[i] - gm[i]) / (2 * hphi);
  RH_ROTOR_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double x0 = k == 0 ? Uinf : (k == 1 ? Omega : pitch_deg);
    const double h = 1e-6 * (fabs(x0) > 1.0 ? fabs(x0) : 1.0);
    const double xp = x0 + h, xm = x0 - h;
    f_and_loads(b, s, phi, rotating, yaw, tilt, azimuth, k == 0 ? xp : Uinf, k == 1 ? xp : Omega, k == 2 ? xp : pitch_deg,
                gp);
    f_and_loads(b, s, phi, rotating, yaw, tilt, azimuth, k == 0 ? xm : Uinf, k == 1 ? xm : Omega, k == 2 ? xm : pitch_deg,
                gm);
    double g_x[3];
    RH_ROTOR_UNROLL
    for (int i = 0; i < 3; ++i) g_x[i] = (gp[i] - gm[i]) / (2 * h);
    const double dphi = (rotating && g_phi[0] != 0) ? -g_x[0] / g_phi[0] : 0.0;
    o.dN[k] = g_x[1] + g_phi[1] * dphi;
    o.dT[k] = g_x[2] + g_phi[2] * dphi;
  }
}

// The terms a section adds to its sector's sums: thrust_torque's integrands times the station's
// trapezoid weight w = 0.5 (ds[i-1] + ds[i]) on the full path (zero loads at the hub and tip
// stations), cone_path the cone angle of that path.  v[0..4] = T, Q, Y, Z, Mflap; v[5..7] = dT/dx,
// v[8..10] = dQ/dx.
constexpr int kSums = 11;
RH_HD inline void section_terms(const PointOut& o, double w, double z_az, double cone_path, double azimuth, double* v) {
  RH_ROTOR_NOFMA
  const double sa = sin(azimuth), ca = cos(azimuth);
  const double scp = sin(cone_path), ccp = cos(cone_path);
  const double radial = o.Np * scp;
  v[0] = w * (o.Np * ccp);
  v[1] = w * (o.Tp * z_az);
  v[2] = w * (o.Tp * ca - radial * sa);
  v[3] = w * (o.Tp * sa + radial * ca);
  v[4] = w * (o.Np * z_az);
  RH_ROTOR_UNROLL
  for (int k = 0; k < 3; ++k) {
    v[5 + k] = w * (o.dN[k] * ccp);
    v[8 + k] = w * (o.dT[k] * z_az);
  }
}

// CCBlade.evaluate's sector combination.  part [nsector][stride]: the kSums sums of each sector (one
// blade at azimuth 360 j / nsector degrees).  loads [8] = T, Y, Z, Q, My, Mz, Mb, P; dloads [6] =
// d(T, Q)/d(Uinf, Omega, pitch) or null.  Returns kNonFinite for a non-finite load.
RH_HD inline int combine_sectors(const double* part, int stride, int nsector, int B, double Omega, double* loads,
                                 double* dloads) {
  RH_ROTOR_NOFMA
  double T = 0, Q = 0, Y = 0, Z = 0, My = 0, Mz = 0, Mb = 0;
  double d[6] = {0, 0, 0, 0, 0, 0};
  for (int j = 0; j < nsector; ++j) {
    const double* p = part + j * stride;
    const double azimuth = (360.0 * (double)j / nsector) * kDeg2Rad;
    const double sa = sin(azimuth), ca = cos(azimuth);
    const double my = p[4] * ca, mz = p[4] * sa;
    T += B * p[0] / nsector;
    Q += B * p[1] / nsector;
    Y += B * p[2] / nsector;
    Z += B * p[3] / nsector;
    My += B * my / nsector;
    Mz += B * mz / nsector;
    Mb += hypot(my, mz) / nsector;
    for (int k = 0; k < 6; ++k) d[k] += B * p[5 + k] / nsector;
  }
  if (nsector == 1) Y = Z = My = Mz = 0.0;   // axisymmetric inflow: the B blades' in-plane loads cancel
  loads[0] = T, loads[1] = Y, loads[2] = Z, loads[3] = Q, loads[4] = My, loads[5] = Mz, loads[6] = Mb;
  loads[7] = Q * Omega * kPi / 30.0;
  bool finite = true;
  for (int k = 0; k < 8; ++k) finite = finite && isfinite(loads[k]);
  if (dloads) {
    for (int k = 0; k < 6; ++k) {
      dloads[k] = d[k];
      finite = finite && isfinite(d[k]);
    }
  }
  return finite ? (int)kOk : (int)kNonFinite;
}

}  // namespace rotor
}  // namespace rh
