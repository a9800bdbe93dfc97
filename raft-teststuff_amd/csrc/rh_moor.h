// rh_moor.h -- quasi-static mooring and the mean-offset Newton, written once for host and device.
//
// FP64 restatement, operation for operation, of raft/mooring.py (catenary, Line.static_solve
// without and with a uniform current, Line.current_load, Body.set_position, body_forces,
// coupled_stiffness_analytic, tensions, coupled_stiffness_fd's tension Jacobian) and of
// Model.solveStatics' eval_func / step_func with raft/dsolve.py's dsolve2.  The same code is
// compiled for gfx950 (rh_moor.hip) and for the CPU check against the Python (tests/test_moor_host.py
// builds tools/moor_host.cpp with g++, tests/test_moor_current_host.py tools/moor_current_host.cpp).
//
// Scope: ONE coupled body whose lines each join one fixed point and one body-attached point,
// W >= 0, with or without a uniform current on the lines (numpy's norm and matrix products may
// differ from the plain C order below in the last bits).  Everything else is refused in
// raft/mooring_device.py.
//
// Lock step: on the device the lines of a case sit in adjacent lanes and the per-case sums go
// through shuffles, so every lane of a wave has to reach them.  Loops therefore run until the
// wave's vote RH_MOOR_ANY says nobody is left, with the updates of finished lanes predicated
// off; a lane's result never depends on its neighbours.  On the host the vote is the lane's own
// flag and the loops are the plain ones of the Python.
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

#if defined(__HIP_DEVICE_COMPILE__)
#define RH_MOOR_ANY(x) (__any((x)) != 0)
#else
#define RH_MOOR_ANY(x) (x)
#endif

#if defined(__clang__)
#define RH_MOOR_UNROLL _Pragma("unroll")
#define RH_MOOR_NOFMA _Pragma("clang fp contract(off)")   // the Python's roundings: no fused multiply-add
#else
#define RH_MOOR_UNROLL
#define RH_MOOR_NOFMA
#endif

namespace rh {
namespace moor {

// per-line / per-case status (0 = fine); a case reports the largest of its lines and its own
enum {
  kOk = 0,
  kXFNegative = 1,          // catenary: XF < 0            (ValueError in raft/mooring.py)
  kLengthNotPositive = 2,   // catenary: L <= 0            (ValueError)
  kEANotPositive = 3,       // catenary: EA <= 0           (ValueError)
  kCatNotConverged = 4,     // catenary: MaxIter reached   (RuntimeError)
  kNewtonNotConverged = 5,  // dsolve2: maxIter evaluations without a step below tol (success = False)
  kSingular = 6,            // the 6 x 6 step matrix has a zero pivot (LinAlgError)
  kBadSystem = 7            // sys_idx outside [0, nsys)
};

constexpr int kCatMaxIter = 100;
constexpr int kNewtonMaxIter = 20;

// (EXF, EZF, J = d(XF, ZF)/d(HF, VF)) of Jonkman's catenary equations (_catenary_residual)
RH_HD inline void catenary_residual(double XF, double ZF, double L, double EA, double W, double CB, double HF, double VF,
                                    double WL, double WEA, double LOvrEA, double CBOvrEA, double& EXF, double& EZF,
                                    double& dXFdHF, double& dXFdVF, double& dZFdHF, double& dZFdVF) {
  RH_MOOR_NOFMA
  const double VFMWL = VF - WL;
  const double HF_W = HF / W;
  const double VF_HF = VF / HF;
  const double VFMWL_HF = VFMWL / HF;
  const double VF_HF2 = VF_HF * VF_HF;
  const double VFMWL_HF2 = VFMWL_HF * VFMWL_HF;
  const double S1 = sqrt(1.0 + VF_HF2);
  const double S2 = sqrt(1.0 + VFMWL_HF2);
  if (CB < 0.0 || VFMWL > 0.0) {   // fully suspended
    const double lg = log(VF_HF + S1) - log(VFMWL_HF + S2);
    EXF = lg * HF_W + LOvrEA * HF - XF;
    EZF = (S1 - S2) * HF_W + LOvrEA * (VF - 0.5 * WL) - ZF;
    dXFdHF = lg / W - ((VF_HF + VF_HF2 / S1) / (VF_HF + S1) - (VFMWL_HF + VFMWL_HF2 / S2) / (VFMWL_HF + S2)) / W + LOvrEA;
    dXFdVF = ((1.0 + VF_HF / S1) / (VF_HF + S1) - (1.0 + VFMWL_HF / S2) / (VFMWL_HF + S2)) / W;
    dZFdHF = (S1 - S2) / W - (VF_HF2 / S1 - VFMWL_HF2 / S2) / W;
    dZFdVF = (VF_HF / S1 - VFMWL_HF / S2) / W + LOvrEA;
  } else if (-CB * VFMWL < HF) {   // on the seabed, anchor tension > 0
    const double LB = L - VF / W;
    const double lg = log(VF_HF + S1);
    EXF = lg * HF_W - 0.5 * CBOvrEA * W * LB * LB + LOvrEA * HF + LB - XF;
    EZF = (S1 - 1.0) * HF_W + 0.5 * VF * VF / WEA - ZF;
    dXFdHF = lg / W - ((VF_HF + VF_HF2 / S1) / (VF_HF + S1)) / W + LOvrEA;
    dXFdVF = ((1.0 + VF_HF / S1) / (VF_HF + S1)) / W + CBOvrEA * LB - 1.0 / W;
    dZFdHF = (S1 - 1.0 - VF_HF2 / S1) / W;
    dZFdVF = (VF_HF / S1) / W + VF / WEA;
  } else {                         // on the seabed, anchor tension 0
    const double LB = L - VF / W;
    const double lg = log(VF_HF + S1);
    const double x = LB - HF_W / CB;
    EXF = lg * HF_W - 0.5 * CBOvrEA * W * (LB * LB - x * x) + LOvrEA * HF + LB - XF;
    EZF = (S1 - 1.0) * HF_W + 0.5 * VF * VF / WEA - ZF;
    dXFdHF = lg / W - ((VF_HF + VF_HF2 / S1) / (VF_HF + S1)) / W + LOvrEA - x / EA;
    dXFdVF = ((1.0 + VF_HF / S1) / (VF_HF + S1)) / W + HF / WEA - 1.0 / W;
    dZFdHF = (S1 - 1.0 - VF_HF2 / S1) / W;
    dZFdVF = (VF_HF / S1) / W + VF / WEA;
  }
}

struct CatOut {
  double HA, VA, HF, VF;        // tension components at the anchor end A and at end B
  double K00, K01, K10, K11;    // d(HF, VF)/d(XF, ZF) = inv(J) at the last evaluated point
  int iters;                    // residual evaluations (both passes of a retried warm start)
  int status;
};

// raft.mooring.catenary.  Newton on (HF, VF) from the warm start (HF0, VF0) > 0 or the Peyrot &
// Goulois guess; dHF is clamped to (Tol - 1) HF; the iteration stops BEFORE applying a step below
// Tol (relative): the returned tensions are the last evaluated point.  A warm start that does not
// converge within kCatMaxIter is retried from the cold guess.  `run` = false lanes (padding)
// only keep the wave's loops company.
RH_HD inline CatOut catenary(double XF, double ZF, double L, double EA, double W, double CB, double Tol, double HF0,
                             double VF0, bool run) {
  RH_MOOR_NOFMA
  CatOut o;
  o.HA = o.VA = o.HF = o.VF = 0.0;
  o.K00 = o.K01 = o.K10 = o.K11 = 0.0;
  o.iters = 0;
  o.status = kOk;
  if (run) {
    if (XF < 0.0) o.status = kXFNegative;
    else if (L <= 0.0) o.status = kLengthNotPositive;
    else if (EA <= 0.0) o.status = kEANotPositive;
  }
  run = run && o.status == kOk;
  const double WL = W * L;
  const double WEA = W * EA;
  const double LOvrEA = L / EA;
  const double CBOvrEA = CB / EA;
  const bool warm = HF0 > 0.0 && VF0 > 0.0;
  bool conv = false;
  double HF = 1.0, VF = 1.0;
  double j00 = 1.0, j01 = 0.0, j10 = 0.0, j11 = 1.0, det = 1.0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const bool go = run && (attempt == 0 || (warm && !conv));
    if (!RH_MOOR_ANY(go)) break;
    if (go) {
      if (attempt == 0 && warm) {
        HF = HF0;
        VF = VF0;
      } else {   // Peyrot & Goulois initial guess (as FAST v7)
        double lam;
        if (XF == 0.0) lam = 1.0e6;
        else if (L <= sqrt(XF * XF + ZF * ZF)) lam = 0.2;
        else lam = sqrt(3.0 * ((L * L - ZF * ZF) / (XF * XF) - 1.0));
        HF = fmax(fabs(0.5 * W * XF / lam), Tol);
        VF = 0.5 * W * (ZF / tanh(lam) + L);
      }
    }
    bool active = go;
    for (int it = 0; it < kCatMaxIter && RH_MOOR_ANY(active); ++it) {
      double EXF, EZF, a00, a01, a10, a11;
      catenary_residual(XF, ZF, L, EA, W, CB, HF, VF, WL, WEA, LOvrEA, CBOvrEA, EXF, EZF, a00, a01, a10, a11);
      if (active) {
        o.iters += 1;
        j00 = a00, j01 = a01, j10 = a10, j11 = a11;
        det = j00 * j11 - j01 * j10;
        double dHF = (-j11 * EXF + j01 * EZF) / det;
        const double dVF = (j10 * EXF - j00 * EZF) / det;
        dHF = fmax(dHF, (Tol - 1.0) * HF);   // keep HF positive
        if (fabs(dHF) <= fabs(Tol * HF) && fabs(dVF) <= fabs(Tol * VF)) {
          conv = true;        // converged: the last (small) step is not applied
          active = false;
        } else {
          HF += dHF;
          VF += dVF;
        }
      }
    }
  }
  if (run && !conv) o.status = kCatNotConverged;
  if (run) {
    o.K00 = j11 / det;
    o.K01 = -j01 / det;
    o.K10 = -j10 / det;
    o.K11 = j00 / det;
    const double VFMWL = VF - WL;
    o.HF = HF;
    o.VF = VF;
    if (CB < 0.0 || VFMWL > 0.0) {
      o.HA = HF;
      o.VA = VFMWL;
    } else if (-CB * VFMWL < HF) {
      o.HA = HF + CB * VFMWL;
      o.VA = 0.0;
    } else {
      o.HA = 0.0;
      o.VA = 0.0;
    }
  }
  return o;
}

// One line of the table: its fixed end (global), its body-attached end (body frame), and which of
// its two ends (A = 0, B = 1) the attached one is.
struct LineIn {
  double fx, fy, fz;
  double ax, ay, az;
  double L, EA, W;
  int att_end;
};

// Line.static_solve (no current) at body pose r6, plus what the body assembly needs.
struct LineSol {
  double rx, ry, rz;            // lever arm of the attached point: p - r6[:3]
  double fx, fy, fz;            // force of the line on the attached point
  double Ku[9];                 // 3 x 3 end stiffness (KA = KB = Ku)
  double TA, TB;                // end tensions |fA|, |fB|
  double HF, VF;                // the catenary's solution: the next warm start
  int iters, status;
};

// rotation_matrix(roll, pitch, yaw) applied to the body-frame point, Body.set_position
RH_HD inline void body_point(const double* r6, double ax, double ay, double az, double& rx, double& ry, double& rz) {
  RH_MOOR_NOFMA
  const double s1 = sin(r6[5]), c1 = cos(r6[5]);
  const double s2 = sin(r6[4]), c2 = cos(r6[4]);
  const double s3 = sin(r6[3]), c3 = cos(r6[3]);
  const double R00 = c1 * c2, R01 = c1 * s2 * s3 - c3 * s1, R02 = s1 * s3 + c1 * c3 * s2;
  const double R10 = c2 * s1, R11 = c1 * c3 + s1 * s2 * s3, R12 = c3 * s1 * s2 - c1 * s3;
  const double R20 = -s2, R21 = c2 * s3, R22 = c2 * c3;
  rx = R00 * ax + R01 * ay + R02 * az;
  ry = R10 * ax + R11 * ay + R12 * az;
  rz = R20 * ax + R21 * ay + R22 * az;
}

// What Line.current_load reads besides the chord: the line type's drag and the case's current.
struct LineCur {
  double d, Cd, CdAx, rho;      // diameter [m], transverse and tangential drag coefficients, water density
  double Ux, Uy, Uz;            // uniform current [m/s], global
};

RH_HD inline void line_solve(const LineIn& ln, bool run, const double* r6, double depth, double tol, double HF0,
                             double VF0, LineSol& s) {
  RH_MOOR_NOFMA
  double qx, qy, qz;
  body_point(r6, ln.ax, ln.ay, ln.az, qx, qy, qz);
  const double px = r6[0] + qx, py = r6[1] + qy, pz = r6[2] + qz;   // the attached point, global
  const bool attA = ln.att_end == 0;
  const double Ax = attA ? px : ln.fx, Ay = attA ? py : ln.fy, Az = attA ? pz : ln.fz;
  const double Bx = attA ? ln.fx : px, By = attA ? ln.fy : py, Bz = attA ? ln.fz : pz;
  const bool swap = Bz < Az;   // the catenary runs from the lower end to the upper one
  const double lx = swap ? Bx : Ax, ly = swap ? By : Ay, lz = swap ? Bz : Az;
  const double ux = swap ? Ax : Bx, uy = swap ? Ay : By, uz = swap ? Az : Bz;
  const double dx = ux - lx, dy = uy - ly, dz = uz - lz;
  const double LH = hypot(dx, dy);
  const double c = LH > 0.0 ? dx / LH : 0.0;
  const double sn = LH > 0.0 ? dy / LH : 0.0;
  const double CB = lz > -depth ? -depth - lz : 0.0;   // off the seabed: no contact
  const CatOut k = catenary(LH, dz, ln.L, ln.EA, ln.W, CB, tol, HF0, VF0, run);
  const double fux = -k.HF * c, fuy = -k.HF * sn, fuz = -k.VF;
  const double flx = k.HA * c, fly = k.HA * sn, flz = k.VA;
  const double Kt = LH > 0.0 ? k.HF / LH : 0.0;   // transverse (geometric) stiffness
  s.Ku[0] = c * c * k.K00 + sn * sn * Kt;
  s.Ku[1] = c * sn * (k.K00 - Kt);
  s.Ku[2] = c * k.K01;
  s.Ku[3] = c * sn * (k.K00 - Kt);
  s.Ku[4] = sn * sn * k.K00 + c * c * Kt;
  s.Ku[5] = sn * k.K01;
  s.Ku[6] = c * k.K10;
  s.Ku[7] = sn * k.K10;
  s.Ku[8] = k.K11;
  const double fAx = swap ? fux : flx, fAy = swap ? fuy : fly, fAz = swap ? fuz : flz;
  const double fBx = swap ? flx : fux, fBy = swap ? fly : fuy, fBz = swap ? flz : fuz;
  s.TA = sqrt(fAx * fAx + fAy * fAy + fAz * fAz);
  s.TB = sqrt(fBx * fBx + fBy * fBy + fBz * fBz);
  s.fx = attA ? fAx : fBx;
  s.fy = attA ? fAy : fBy;
  s.fz = attA ? fAz : fBz;
  s.rx = px - r6[0];
  s.ry = py - r6[1];
  s.rz = pz - r6[2];
  s.HF = k.HF;
  s.VF = k.VF;
  s.iters = k.iters;
  s.status = k.status;
  const bool ok = run && (k.status == kOk || k.status == kCatNotConverged);
  if (!ok) {   // padding lanes and refused lines contribute zeros
    s.fx = s.fy = s.fz = 0.0;
    s.TA = s.TB = 0.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 9; ++i) s.Ku[i] = 0.0;
    s.HF = s.VF = 0.0;
  }
}

// Line.static_solve(current=U) at body pose r6: line_solve with the current branch.  The wet
// weight plus Line.current_load on the chord at THIS pose is the distributed load (so the central
// differences of the tension Jacobian re-evaluate the drag on each perturbed chord, as
// coupled_stiffness_fd does by calling static_solve again); the catenary is solved with
// W' = |load| in the frame R whose -z axis is the load's direction, and forces and stiffness are
// rotated back.  A lane whose current is exactly (0, 0, 0) takes line_solve's values through
// selects, bit for bit (np.any(current) is false in the Python); the current / no-current and
// the up / no-up choices are selects, never early exits, so every lane reaches the catenary's
// votes.  (A function of its own, not a variant of line_solve: the kernels without current keep
// their instructions.)
// branch: bit 0 = the current branch was taken, bit 1 = the load points up (R0 applied, CB = -1).
RH_HD inline void line_solve_current(const LineIn& ln, const LineCur& cu, bool run, const double* r6, double depth,
                                     double tol, double HF0, double VF0, LineSol& s, int& branch) {
  RH_MOOR_NOFMA
  double qx, qy, qz;
  body_point(r6, ln.ax, ln.ay, ln.az, qx, qy, qz);
  const double px = r6[0] + qx, py = r6[1] + qy, pz = r6[2] + qz;   // the attached point, global
  const bool attA = ln.att_end == 0;
  const double Ax = attA ? px : ln.fx, Ay = attA ? py : ln.fy, Az = attA ? pz : ln.fz;
  const double Bx = attA ? ln.fx : px, By = attA ? ln.fy : py, Bz = attA ? ln.fz : pz;
  const bool cur = cu.Ux != 0.0 || cu.Uy != 0.0 || cu.Uz != 0.0;
  // current_load: transverse and tangential drag per unit length on the chord A -> B
  const double ex = Bx - Ax, ey = By - Ay, ez = Bz - Az;
  const double en = sqrt(ex * ex + ey * ey + ez * ez);
  const double tx = en > 0.0 ? ex / en : 0.0, ty = en > 0.0 ? ey / en : 0.0, tz = en > 0.0 ? ez / en : 1.0;
  const double ut = cu.Ux * tx + cu.Uy * ty + cu.Uz * tz;
  const double Utx = ut * tx, Uty = ut * ty, Utz = ut * tz;
  const double Unx = cu.Ux - Utx, Uny = cu.Uy - Uty, Unz = cu.Uz - Utz;
  const double kn = 0.5 * cu.rho * cu.d * cu.Cd * sqrt(Unx * Unx + Uny * Uny + Unz * Unz);
  const double kt = 0.5 * cu.rho * 3.141592653589793 * cu.d * cu.CdAx * sqrt(Utx * Utx + Uty * Uty + Utz * Utz);
  // the distributed load (0, 0, -W) + drag, its size W' and its direction a
  const double f0 = 0.0 + (kn * Unx + kt * Utx);
  const double f1 = 0.0 + (kn * Uny + kt * Uty);
  const double f2 = -ln.W + (kn * Unz + kt * Utz);
  const double Wc = sqrt(f0 * f0 + f1 * f1 + f2 * f2);
  const double W = cur ? Wc : ln.W;
  const double a0 = f0 / Wc, a1r = f1 / Wc, a2r = f2 / Wc;
  const bool up = cur && a2r > 0.0;   // the net load points away from the seabed
  // a load with an upward component is first turned 180 deg about x (R0 = diag(1, -1, -1)), so
  // that the Rodrigues step is taken at 1 + cos >= 1
  const double a1 = up ? -a1r : a1r, a2 = up ? -a2r : a2r;
  const double v0 = a1 * -1.0 - a2 * 0.0, v1 = a2 * 0.0 - a0 * -1.0;   // a x (0, 0, -1)
  const double den = 1.0 + (-a2);
  // R = (I + V + V V / (1 + cos)) R0, V the cross-product matrix of v = (v0, v1, 0): R a = (0, 0, -1)
  const double r01 = (v1 * v0) / den, r10 = (v0 * v1) / den;
  const double r11 = 1.0 + (-(v0 * v0)) / den, r22 = 1.0 + (-(v1 * v1) - v0 * v0) / den;
  const double R[9] = {1.0 + (-(v1 * v1)) / den, up ? -r01 : r01, up ? -v1 : v1,
                       r10, up ? -r11 : r11, up ? v0 : -v0,
                       -v1, up ? -v0 : v0, up ? -r22 : r22};
  // the ends are ordered by height along the load
  const double zA = cur ? R[6] * Ax + R[7] * Ay + R[8] * Az : Az;
  const double zB = cur ? R[6] * Bx + R[7] * By + R[8] * Bz : Bz;
  const bool swap = zB < zA;   // the catenary runs from the lower end to the upper one
  const double lx = swap ? Bx : Ax, ly = swap ? By : Ay, lz = swap ? Bz : Az;
  const double ux = swap ? Ax : Bx, uy = swap ? Ay : By, uz = swap ? Az : Bz;
  const double gx = ux - lx, gy = uy - ly, gz = uz - lz;
  const double dx = cur ? R[0] * gx + R[1] * gy + R[2] * gz : gx;
  const double dy = cur ? R[3] * gx + R[4] * gy + R[5] * gz : gy;
  const double dz = cur ? R[6] * gx + R[7] * gy + R[8] * gz : gz;
  const double LH = hypot(dx, dy);
  const double c = LH > 0.0 ? dx / LH : 0.0;
  const double sn = LH > 0.0 ? dy / LH : 0.0;
  // off the seabed: no contact (the global depth of the end that ordering calls lower); pulled
  // away from the seabed: never in contact
  const double CB = up ? -1.0 : lz > -depth ? -depth - lz : 0.0;
  const CatOut k = catenary(LH, dz, ln.L, ln.EA, W, CB, tol, HF0, VF0, run);
  const double hux = -k.HF * c, huy = -k.HF * sn, huz = -k.VF;
  const double hlx = k.HA * c, hly = k.HA * sn, hlz = k.VA;
  const double Kt = LH > 0.0 ? k.HF / LH : 0.0;   // transverse (geometric) stiffness
  const double Kl[9] = {c * c * k.K00 + sn * sn * Kt, c * sn * (k.K00 - Kt), c * k.K01,
                        c * sn * (k.K00 - Kt), sn * sn * k.K00 + c * c * Kt, sn * k.K01,
                        c * k.K10, sn * k.K10, k.K11};
  // back to the global frame: R' f and R' Ku R
  const double fux = cur ? R[0] * hux + R[3] * huy + R[6] * huz : hux;
  const double fuy = cur ? R[1] * hux + R[4] * huy + R[7] * huz : huy;
  const double fuz = cur ? R[2] * hux + R[5] * huy + R[8] * huz : huz;
  const double flx = cur ? R[0] * hlx + R[3] * hly + R[6] * hlz : hlx;
  const double fly = cur ? R[1] * hlx + R[4] * hly + R[7] * hlz : hly;
  const double flz = cur ? R[2] * hlx + R[5] * hly + R[8] * hlz : hlz;
  double M[9];   // R' Ku
  RH_MOOR_UNROLL
  for (int i = 0; i < 3; ++i) {
    RH_MOOR_UNROLL
    for (int j = 0; j < 3; ++j) M[3 * i + j] = R[i] * Kl[j] + R[3 + i] * Kl[3 + j] + R[6 + i] * Kl[6 + j];
  }
  RH_MOOR_UNROLL
  for (int i = 0; i < 3; ++i) {
    RH_MOOR_UNROLL
    for (int j = 0; j < 3; ++j) {
      const double g = M[3 * i] * R[j] + M[3 * i + 1] * R[3 + j] + M[3 * i + 2] * R[6 + j];
      s.Ku[3 * i + j] = cur ? g : Kl[3 * i + j];
    }
  }
  branch = (cur ? 1 : 0) | (up ? 2 : 0);
  const double fAx = swap ? fux : flx, fAy = swap ? fuy : fly, fAz = swap ? fuz : flz;
  const double fBx = swap ? flx : fux, fBy = swap ? fly : fuy, fBz = swap ? flz : fuz;
  s.TA = sqrt(fAx * fAx + fAy * fAy + fAz * fAz);
  s.TB = sqrt(fBx * fBx + fBy * fBy + fBz * fBz);
  s.fx = attA ? fAx : fBx;
  s.fy = attA ? fAy : fBy;
  s.fz = attA ? fAz : fBz;
  s.rx = px - r6[0];
  s.ry = py - r6[1];
  s.rz = pz - r6[2];
  s.HF = k.HF;
  s.VF = k.VF;
  s.iters = k.iters;
  s.status = k.status;
  const bool ok = run && (k.status == kOk || k.status == kCatNotConverged);
  if (!ok) {   // padding lanes and refused lines contribute zeros
    s.fx = s.fy = s.fz = 0.0;
    s.TA = s.TB = 0.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 9; ++i) s.Ku[i] = 0.0;
    s.HF = s.VF = 0.0;
  }
}

// body_forces(lines_only=True) of one line: (f, r x f)
RH_HD inline void line_force6(const LineSol& s, double* F) {
  RH_MOOR_NOFMA
  F[0] = s.fx;
  F[1] = s.fy;
  F[2] = s.fz;
  F[3] = s.ry * s.fz - s.rz * s.fy;
  F[4] = s.rz * s.fx - s.rx * s.fz;
  F[5] = s.rx * s.fy - s.ry * s.fx;
}

// coupled_stiffness_analytic() of one line, row-major 6 x 6: T' Ku T with T = [I, H(r)], plus the
// geometric term -H(f) H(r) of the attachment force on the rotational block.
// H(v) = get_h(v): H(v) u = u x v.
RH_HD inline void line_stiffness36(const LineSol& s, double* K) {
  RH_MOOR_NOFMA
  const double Hr[9] = {0.0, s.rz, -s.ry, -s.rz, 0.0, s.rx, s.ry, -s.rx, 0.0};
  const double Hf[9] = {0.0, s.fz, -s.fy, -s.fz, 0.0, s.fx, s.fy, -s.fx, 0.0};
  double KH[9];   // Ku H(r)
  RH_MOOR_UNROLL
  for (int i = 0; i < 3; ++i) {
    RH_MOOR_UNROLL
    for (int j = 0; j < 3; ++j)
      KH[3 * i + j] = s.Ku[3 * i] * Hr[j] + s.Ku[3 * i + 1] * Hr[3 + j] + s.Ku[3 * i + 2] * Hr[6 + j];
  }
  RH_MOOR_UNROLL
  for (int i = 0; i < 3; ++i) {
    RH_MOOR_UNROLL
    for (int j = 0; j < 3; ++j) {
      K[6 * i + j] = s.Ku[3 * i + j];
      K[6 * i + 3 + j] = KH[3 * i + j];
      // H(r)' Ku
      K[6 * (3 + i) + j] = Hr[i] * s.Ku[j] + Hr[3 + i] * s.Ku[3 + j] + Hr[6 + i] * s.Ku[6 + j];
      // H(r)' Ku H(r) - H(f) H(r)
      K[6 * (3 + i) + 3 + j] = (Hr[i] * KH[j] + Hr[3 + i] * KH[3 + j] + Hr[6 + i] * KH[6 + j]) -
                               (Hf[3 * i] * Hr[j] + Hf[3 * i + 1] * Hr[3 + j] + Hf[3 * i + 2] * Hr[6 + j]);
    }
  }
}

// A x = b, 6 x 6, partially pivoted real LU (np.linalg.solve), fully unrolled.  The pivot row is
// brought up by compare-and-swap of whole rows, so no index depends on data.  false = zero pivot.
RH_HD inline bool solve6(const double* A, const double* b, double* x) {
  RH_MOOR_NOFMA
  double a[6][7];
  RH_MOOR_UNROLL
  for (int i = 0; i < 6; ++i) {
    RH_MOOR_UNROLL
    for (int j = 0; j < 6; ++j) a[i][j] = A[6 * i + j];
    a[i][6] = b[i];
  }
  bool ok = true;
  RH_MOOR_UNROLL
  for (int k = 0; k < 6; ++k) {
    RH_MOOR_UNROLL
    for (int i = k + 1; i < 6; ++i) {
      const bool sw = fabs(a[i][k]) > fabs(a[k][k]);
      RH_MOOR_UNROLL
      for (int j = k; j < 7; ++j) {
        const double t = a[k][j];
        a[k][j] = sw ? a[i][j] : t;
        a[i][j] = sw ? t : a[i][j];
      }
    }
    ok = ok && a[k][k] != 0.0;
    RH_MOOR_UNROLL
    for (int i = k + 1; i < 6; ++i) {
      const double m = a[i][k] / a[k][k];
      RH_MOOR_UNROLL
      for (int j = k + 1; j < 7; ++j) a[i][j] -= m * a[k][j];
    }
  }
  RH_MOOR_UNROLL
  for (int i = 5; i >= 0; --i) {
    double v = a[i][6];
    RH_MOOR_UNROLL
    for (int j = i + 1; j < 6; ++j) v -= a[i][j] * x[j];
    x[i] = v / a[i][i];
  }
  return ok;
}

// Model.solveStatics (statics_mod 0, forcing_mod 0) for one FOWT with its own mooring system:
//   eval_func  Fnet = F_const - K_hs (X - X_ref) + F_moor(X)
//   step_func  K = K_hs + C_moor(X); a zero diagonal entry becomes the mean diagonal; dX = K^-1 Fnet;
//              at most ten 10 % diagonal strengthenings while dX . Fnet < 0
//   dsolve2    a step that re-crosses the plane at 0.62 of the previous step back is scaled onto it;
//              converged when every |dX_i| < tol_i = [0.05]*3 + [0.005]*3, that step NOT applied;
//              at most kNewtonMaxIter evaluations.
// ev(X, F, K) evaluates the mooring at pose X: F [6], K [36] row-major, returns a status; it
// carries the catenary warm state from one evaluation to the next, and every lane of a case
// gets the same F, K and status back.  `live` = false lanes only keep the wave company.
template <class Eval>
RH_HD inline void statics_newton(Eval& ev, bool live, const double* X_ref, const double* K_hs, const double* F_const,
                                 double* X, int& iters, int& status) {
  RH_MOOR_NOFMA
  double dXl[6];
  RH_MOOR_UNROLL
  for (int i = 0; i < 6; ++i) {
    X[i] = X_ref[i];
    dXl[i] = 0.0;
  }
  iters = 0;
  status = live ? kNewtonNotConverged : kOk;
  for (int it = 0; it < kNewtonMaxIter && RH_MOOR_ANY(live); ++it) {
    double F[6], K[36];
    const int st = ev(X, F, K);
    if (live) {
      iters += 1;
      if (st != kOk) {
        status = st;
        live = false;
      } else if (it == kNewtonMaxIter - 1) {
        live = false;
      }
    }
    double Y[6], dX[6];
    RH_MOOR_UNROLL
    for (int i = 0; i < 6; ++i) {
      double kx = 0.0;
      RH_MOOR_UNROLL
      for (int j = 0; j < 6; ++j) kx += K_hs[6 * i + j] * (X[j] - X_ref[j]);
      Y[i] = F_const[i] + (-kx) + F[i];
    }
    double ksum = 0.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 36; ++i) K[i] += K_hs[i];
    RH_MOOR_UNROLL
    for (int i = 0; i < 6; ++i) ksum += K[7 * i];
    const double kmean = ksum / 6.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 6; ++i)
      if (K[7 * i] == 0.0) K[7 * i] = kmean;
    bool ok = solve6(K, Y, dX);
    for (int r = 0; r < 10; ++r) {   // strengthen the diagonal on a backward step
      double dot = 0.0;
      RH_MOOR_UNROLL
      for (int i = 0; i < 6; ++i) dot += dX[i] * Y[i];
      const bool back = live && ok && dot < 0.0;
      if (!RH_MOOR_ANY(back)) break;
      if (back) {
        RH_MOOR_UNROLL
        for (int i = 0; i < 6; ++i) K[7 * i] += 0.1 * fabs(K[7 * i]);
      }
      double d2[6];
      const bool ok2 = solve6(K, Y, d2);
      if (back) {
        ok = ok2;
        RH_MOOR_UNROLL
        for (int i = 0; i < 6; ++i) dX[i] = d2[i];
      }
    }
    if (live && !ok) {
      status = kSingular;
      live = false;
    }
    // dsolve2: do not re-cross the plane at 0.62 of the previous step back
    double lhs = 0.0, rhs = 0.0, num = 0.0, den = 0.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 6; ++i) {
      const double xlim = X[i] - 0.62 * dXl[i];
      lhs += (X[i] + dX[i]) * dXl[i];
      rhs += xlim * dXl[i];
      num += (xlim - X[i]) * dXl[i];
      den += dX[i] * dXl[i];
    }
    if (lhs < rhs) {
      const double alpha = num / den;
      RH_MOOR_UNROLL
      for (int i = 0; i < 6; ++i) dX[i] = alpha * dX[i];
    }
    bool small = true;
    RH_MOOR_UNROLL
    for (int i = 0; i < 6; ++i) small = small && fabs(dX[i]) < (i < 3 ? 0.05 : 0.005);
    if (live) {
      if (small) {   // converged: the step is not applied
        status = kOk;
        live = false;
      } else {
        RH_MOOR_UNROLL
        for (int i = 0; i < 6; ++i) {
          dXl[i] = dX[i];
          X[i] = X[i] + dX[i];
        }
      }
    }
  }
}

}  // namespace moor
}  // namespace rh
