// rh_moor_array.h -- a general quasi-static mooring system (several bodies, free points, shared
// lines) and the mean-offset Newton of N FOWTs on it, written once for host and device.
//
// FP64 restatement of raft/mooring.py (Line.static_solve without current for two arbitrary ends,
// MooringSystem.solve_equilibrium with raft/dsolve.py's dsolve2 on the free points, point_force,
// body_forces, coupled_stiffness_analytic with the free points condensed out, tensions, the
// tension Jacobian of coupled_stiffness_fd) and of Model.solveStatics' eval_func / step_func for
// N FOWTs.  The single-body code of rh_moor.h is used as it is (catenary, body_point) and not
// changed.  Compiled for gfx950 by rh_moor_array.hip and for the CPU check against the Python by
// tools/moor_array_host.cpp (tests/test_moor_array_host.py).
//
// One flattened record (ArrSys) holds everything a model's statics see: a point table (kind,
// body or free index, xyz, mass, volume), a line table (point A, point B, L, EA, W, and the depth
// and catenary tolerance of the system the line came from) and the system each line belongs to.
// Free points live in ONE of the merged systems (free_sys): separate systems are separate dsolve2
// problems on the host, so only that system's lines are solved again inside the free-point Newton.
//
// Execution: the per-line work (end positions, catenary, end forces, Ku) is done for lines
// [ex.lbeg, ex.lend): every line in turn on the host, the lane's own line on the device.  The dense
// work (free-point matrix, condensation, the 6nb x 6nb step) is done by ex.leader alone, line after
// line in table order, on a per-pose workspace (LDS on the device) that ex.sync() makes visible.
// So the sums of a pose have one fixed order that depends on nothing outside the pose.
// Lock step as in rh_moor.h: every loop that holds a vote or a sync runs to the wave's vote
// RH_MOOR_ANY with finished poses predicated off, and no branch around a vote or a sync depends on
// anything but such votes and launch-wide arguments.  The device runs one wave per workgroup.
#pragma once
#include "rh_moor.h"

namespace rh {
namespace moor {

enum {
  kFreeNotConverged = 8,   // solve_equilibrium: 500 evaluations without a step below free_tol
  kFreeSingular = 9        // zero pivot in the free-point matrix (Newton step or condensation)
};

constexpr int kFreeMaxIter = 500;
// (limits of a record: RH_MOOR_MAX_BODIES, RH_MOOR_MAX_FREE, RH_MOOR_MAX_LINES of include/rafthip.h)

// point-table rows / line-table rows (struct of arrays, enum rh_moor_point_field / rh_moor_aline_field)
enum { kPtKind = 0, kPtIndex, kPtX, kPtY, kPtZ, kPtM, kPtV, kPtCount };
enum { kLnA = 0, kLnB, kLnL, kLnEA, kLnW, kLnDepth, kLnTol, kLnSys, kLnCount };
enum { kFixed = 0, kOnBody = 1, kFree = 2 };

struct ArrSys {
  int nb, np, nl, nf;     // bodies, points, lines, free points
  int free_sys;           // the system (membership value) that holds the free points, or -1
  double g, rho;          // of the system with the free points (their weight and buoyancy)
  double free_tol;        // MooringSystem.free_tol
  double free_depth;      // its depth: the free-point step is capped at depth / 10
  const double* pt;       // [kPtCount][np]
  const double* ln;       // [kLnCount][nl]
};

// per-line results kept in the workspace: fA[3], fB[3], Ku[9], rA[3], rB[3] (lever arms of
// body-attached ends, p - r6[:3])
constexpr int kLo = 21;

// The per-pose workspace, laid out for the call's largest nD = 6 nb, nF = 3 nfree and nl.
struct ArrWs {
  double *X, *dXl, *Y, *dX;          // [nD] pose, last step, net force, step
  double *fp, *fdXl, *fY, *fp0;      // [nF] free points, their last step, their net force, a saved copy
  double *Fb, *Kb;                   // [nD], [nD nD] mooring force and stiffness of the body DOFs
  double *Bm;                        // [nD nF]  T' Kaf
  double *A;                         // [max(nF (nF + nD), nD (nD + 1))] LU work array
  double *lo;                        // [nl kLo]
  double *wHF, *wVF, *w0HF, *w0VF;   // [nl] catenary warm state and a saved copy
  double *TA, *TB, *TpA, *TpB;       // [nl] end tensions and a saved copy
  double *lst;                       // [nl] the largest status of each line
  double *flag;                      // [4] go-on flag, status, evaluation count, spare
};

RH_HD inline int arr_ws_doubles(int nD, int nF, int nl) {
  const int a1 = nF * (nF + nD), a2 = nD * (nD + 1);
  return 4 * nD + 4 * nF + nD + nD * nD + nD * nF + (a1 > a2 ? a1 : a2) + nl * kLo + 9 * nl + 4;
}

RH_HD inline void arr_ws_carve(double* p, int nD, int nF, int nl, ArrWs& w) {
  const int a1 = nF * (nF + nD), a2 = nD * (nD + 1);
  w.X = p, p += nD;
  w.dXl = p, p += nD;
  w.Y = p, p += nD;
  w.dX = p, p += nD;
  w.fp = p, p += nF;
  w.fdXl = p, p += nF;
  w.fY = p, p += nF;
  w.fp0 = p, p += nF;
  w.Fb = p, p += nD;
  w.Kb = p, p += nD * nD;
  w.Bm = p, p += nD * nF;
  w.A = p, p += (a1 > a2 ? a1 : a2);
  w.lo = p, p += nl * kLo;
  w.wHF = p, p += nl;
  w.wVF = p, p += nl;
  w.w0HF = p, p += nl;
  w.w0VF = p, p += nl;
  w.TA = p, p += nl;
  w.TB = p, p += nl;
  w.TpA = p, p += nl;
  w.TpB = p, p += nl;
  w.lst = p, p += nl;
  w.flag = p;
}

RH_HD inline int arr_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? (n > 0 ? n - 1 : 0) : v); }

// Global position of point ip at body poses X and free-point positions fp; the lever arm of a
// body-attached point.  Indices are clamped into range (the host validates the tables).
RH_HD inline void arr_point(const ArrSys& S, int ip, const double* X, const double* fp, double& x, double& y, double& z,
                            int& kind, int& idx, double& rx, double& ry, double& rz) {
  RH_MOOR_NOFMA
  ip = arr_clampi(ip, S.np);
  kind = (int)S.pt[kPtKind * S.np + ip];
  idx = (int)S.pt[kPtIndex * S.np + ip];
  const double px = S.pt[kPtX * S.np + ip], py = S.pt[kPtY * S.np + ip], pz = S.pt[kPtZ * S.np + ip];
  rx = ry = rz = 0.0;
  if (kind == kOnBody) {
    idx = arr_clampi(idx, S.nb);
    const double* r6 = X + 6 * idx;
    double qx, qy, qz;
    body_point(r6, px, py, pz, qx, qy, qz);
    x = r6[0] + qx, y = r6[1] + qy, z = r6[2] + qz;
    rx = x - r6[0], ry = y - r6[1], rz = z - r6[2];
  } else if (kind == kFree) {
    idx = arr_clampi(idx, S.nf);
    x = fp[3 * idx], y = fp[3 * idx + 1], z = fp[3 * idx + 2];
  } else {
    kind = kFixed;
    x = px, y = py, z = pz;
  }
}

struct ALineSol {
  double fA[3], fB[3];   // force of the line on its end points
  double Ku[9];          // KA = KB = Ku, KAB = -Ku
  double TA, TB, HF, VF;
  int iters, status;
};

// Line.static_solve (no current) for two arbitrary end positions: ends ordered by height, CB
// from the lower end and this line's depth.
RH_HD inline void arr_line_solve(double Ax, double Ay, double Az, double Bx, double By, double Bz, double L, double EA,
                                 double W, double depth, double tol, double HF0, double VF0, bool run, ALineSol& s) {
  RH_MOOR_NOFMA
  const bool swap = Bz < Az;
  const double lx = swap ? Bx : Ax, ly = swap ? By : Ay, lz = swap ? Bz : Az;
  const double ux = swap ? Ax : Bx, uy = swap ? Ay : By, uz = swap ? Az : Bz;
  const double dx = ux - lx, dy = uy - ly, dz = uz - lz;
  const double LH = hypot(dx, dy);
  const double c = LH > 0.0 ? dx / LH : 0.0;
  const double sn = LH > 0.0 ? dy / LH : 0.0;
  const double CB = lz > -depth ? -depth - lz : 0.0;
  const CatOut k = catenary(LH, dz, L, EA, W, CB, tol, HF0, VF0, run);
  const double fux = -k.HF * c, fuy = -k.HF * sn, fuz = -k.VF;
  const double flx = k.HA * c, fly = k.HA * sn, flz = k.VA;
  const double Kt = LH > 0.0 ? k.HF / LH : 0.0;
  s.Ku[0] = c * c * k.K00 + sn * sn * Kt;
  s.Ku[1] = c * sn * (k.K00 - Kt);
  s.Ku[2] = c * k.K01;
  s.Ku[3] = c * sn * (k.K00 - Kt);
  s.Ku[4] = sn * sn * k.K00 + c * c * Kt;
  s.Ku[5] = sn * k.K01;
  s.Ku[6] = c * k.K10;
  s.Ku[7] = sn * k.K10;
  s.Ku[8] = k.K11;
  s.fA[0] = swap ? fux : flx, s.fA[1] = swap ? fuy : fly, s.fA[2] = swap ? fuz : flz;
  s.fB[0] = swap ? flx : fux, s.fB[1] = swap ? fly : fuy, s.fB[2] = swap ? flz : fuz;
  s.TA = sqrt(s.fA[0] * s.fA[0] + s.fA[1] * s.fA[1] + s.fA[2] * s.fA[2]);
  s.TB = sqrt(s.fB[0] * s.fB[0] + s.fB[1] * s.fB[1] + s.fB[2] * s.fB[2]);
  s.HF = k.HF;
  s.VF = k.VF;
  s.iters = k.iters;
  s.status = k.status;
  const bool ok = run && (k.status == kOk || k.status == kCatNotConverged);
  if (!ok) {   // padding lanes and refused lines contribute zeros
    RH_MOOR_UNROLL
    for (int i = 0; i < 3; ++i) s.fA[i] = s.fB[i] = 0.0;
    RH_MOOR_UNROLL
    for (int i = 0; i < 9; ++i) s.Ku[i] = 0.0;
    s.TA = s.TB = s.HF = s.VF = 0.0;
  }
}

// _solve_lines: every line of the record (all = true) or the lines of the free-point system only,
// at the poses and free points of the workspace.  Results go to the workspace.
template <class Ex>
RH_HD inline void arr_solve_lines(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, bool all) {
  RH_MOOR_NOFMA
  for (int l = ex.lbeg; l < ex.lend; ++l) {
    const bool has = l < S.nl;
    const int ll = has ? l : S.nl - 1;   // padding lanes read the last line (in bounds) and discard it
    const int iA = (int)S.ln[kLnA * S.nl + ll], iB = (int)S.ln[kLnB * S.nl + ll];
    const bool mine = all || (int)S.ln[kLnSys * S.nl + ll] == S.free_sys;
    const bool run = live && has && mine;
    double Ax, Ay, Az, Bx, By, Bz, rA[3], rB[3];
    int kA, jA, kB, jB;
    arr_point(S, iA, w.X, w.fp, Ax, Ay, Az, kA, jA, rA[0], rA[1], rA[2]);
    arr_point(S, iB, w.X, w.fp, Bx, By, Bz, kB, jB, rB[0], rB[1], rB[2]);
    ALineSol s;
    arr_line_solve(Ax, Ay, Az, Bx, By, Bz, S.ln[kLnL * S.nl + ll], S.ln[kLnEA * S.nl + ll], S.ln[kLnW * S.nl + ll],
                   S.ln[kLnDepth * S.nl + ll], S.ln[kLnTol * S.nl + ll], run ? w.wHF[ll] : 0.0, run ? w.wVF[ll] : 0.0, run,
                   s);
    if (run) {
      double* o = w.lo + kLo * l;
      for (int i = 0; i < 3; ++i) o[i] = s.fA[i], o[3 + i] = s.fB[i], o[15 + i] = rA[i], o[18 + i] = rB[i];
      for (int i = 0; i < 9; ++i) o[6 + i] = s.Ku[i];
      w.wHF[l] = s.HF;
      w.wVF[l] = s.VF;
      w.TA[l] = s.TA;
      w.TB[l] = s.TB;
      if ((double)s.status > w.lst[l]) w.lst[l] = (double)s.status;
    }
  }
}

// In-place partially pivoted LU solve (np.linalg.solve) of the n x n system held in the first n
// columns of M (row stride ld) for the nrhs right-hand sides in the columns after them.
// false = zero pivot.
RH_HD inline bool arr_lu_solve(double* M, int n, int nrhs, int ld) {
  RH_MOOR_NOFMA
  bool ok = true;
  const int nc = n + nrhs;
  for (int k = 0; k < n; ++k) {
    int p = k;
    double big = fabs(M[k * ld + k]);
    for (int i = k + 1; i < n; ++i) {
      const double v = fabs(M[i * ld + k]);
      if (v > big) big = v, p = i;
    }
    if (p != k)
      for (int j = 0; j < nc; ++j) {
        const double t = M[k * ld + j];
        M[k * ld + j] = M[p * ld + j];
        M[p * ld + j] = t;
      }
    const double piv = M[k * ld + k];
    ok = ok && piv != 0.0;
    for (int i = k + 1; i < n; ++i) {
      const double m = M[i * ld + k] / piv;
      for (int j = k + 1; j < nc; ++j) M[i * ld + j] -= m * M[k * ld + j];
    }
  }
  for (int r = 0; r < nrhs; ++r)
    for (int i = n - 1; i >= 0; --i) {
      double v = M[i * ld + n + r];
      for (int j = i + 1; j < n; ++j) v -= M[i * ld + j] * M[j * ld + n + r];
      M[i * ld + n + r] = v / M[i * ld + i];
    }
  return ok;
}

// kind and index (body or free) of a line's two end points
RH_HD inline void arr_line_ends(const ArrSys& S, int l, int& kA, int& jA, int& kB, int& jB) {
  const int iA = arr_clampi((int)S.ln[kLnA * S.nl + l], S.np), iB = arr_clampi((int)S.ln[kLnB * S.nl + l], S.np);
  kA = (int)S.pt[kPtKind * S.np + iA];
  kB = (int)S.pt[kPtKind * S.np + iB];
  jA = arr_clampi((int)S.pt[kPtIndex * S.np + iA], kA == kFree ? S.nf : S.nb);
  jB = arr_clampi((int)S.pt[kPtIndex * S.np + iB], kB == kFree ? S.nf : S.nb);
}

// dst[3 ia + i][3 ib + j] += sgn * (tr ? K[j][i] : K[i][j]); dst has row stride ld
RH_HD inline void arr_add33(double* dst, int ld, int ia, int ib, const double* K, double sgn, bool tr) {
  RH_MOOR_NOFMA
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) dst[(3 * ia + i) * ld + 3 * ib + j] += sgn * (tr ? K[3 * j + i] : K[3 * i + j]);
}

// The free points' net force fY (lines, weight and buoyancy) and their stiffness _free_stiffness
// into the first nF columns of w.A (row stride ld).  Leader only.
RH_HD inline void arr_free_assemble(const ArrSys& S, const ArrWs& w, int ld) {
  RH_MOOR_NOFMA
  const int nF = 3 * S.nf;
  for (int i = 0; i < nF; ++i) {
    w.fY[i] = 0.0;
    for (int j = 0; j < nF; ++j) w.A[i * ld + j] = 0.0;
  }
  for (int l = 0; l < S.nl; ++l) {
    int kA, jA, kB, jB;
    arr_line_ends(S, l, kA, jA, kB, jB);
    const double* o = w.lo + kLo * l;
    if (kA == kFree) {
      for (int i = 0; i < 3; ++i) w.fY[3 * jA + i] += o[i];
      arr_add33(w.A, ld, jA, jA, o + 6, 1.0, false);
    }
    if (kB == kFree) {
      for (int i = 0; i < 3; ++i) w.fY[3 * jB + i] += o[3 + i];
      arr_add33(w.A, ld, jB, jB, o + 6, 1.0, false);
    }
    if (kA == kFree && kB == kFree) {
      arr_add33(w.A, ld, jA, jB, o + 6, -1.0, false);
      arr_add33(w.A, ld, jB, jA, o + 6, -1.0, true);
    }
  }
  for (int ip = 0; ip < S.np; ++ip)
    if ((int)S.pt[kPtKind * S.np + ip] == kFree) {
      const int j = arr_clampi((int)S.pt[kPtIndex * S.np + ip], S.nf);
      w.fY[3 * j + 2] += -S.pt[kPtM * S.np + ip] * S.g + S.pt[kPtV * S.np + ip] * S.rho * S.g;
    }
}

// MooringSystem.solve_equilibrium at the workspace's poses: every line once, then dsolve2 on the
// free-point coordinates (Newton on _free_stiffness, the step capped at depth / 10, tolerance
// free_tol, at most kFreeMaxIter evaluations, the converging step not applied) and one more
// evaluation at the returned point.  `nev` counts the line passes (_solve_lines calls) of a live
// pose; `st` collects kFreeNotConverged / kFreeSingular.
template <class Ex>
RH_HD inline void arr_equilibrium(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, int& nev, int& st) {
  RH_MOOR_NOFMA
  arr_solve_lines(S, ex, w, live, true);
  if (live) nev += 1;
  const int nF = 3 * S.nf;
  const int ld = nF + 1;
  const bool fr = live && S.nf > 0;
  if (ex.leader && fr)
    for (int i = 0; i < nF; ++i) w.fdXl[i] = 0.0;
  ex.sync();
  bool go = fr;
  for (int it = 0; it < kFreeMaxIter && RH_MOOR_ANY(go); ++it) {
    arr_solve_lines(S, ex, w, go, false);
    if (go) nev += 1;
    ex.sync();
    if (ex.leader && go) {
      double flag = 1.0, stat = 0.0;
      arr_free_assemble(S, w, ld);
      if (it == kFreeMaxIter - 1) {
        flag = 0.0;
        stat = (double)kFreeNotConverged;
      } else {
        for (int i = 0; i < nF; ++i) w.A[i * ld + nF] = w.fY[i];
        if (!arr_lu_solve(w.A, nF, 1, ld)) {
          flag = 0.0;
          stat = (double)kFreeSingular;
        } else {
          const double lim = S.free_depth > 0.0 ? S.free_depth / 10 : 10.0;
          double big = 0.0;
          for (int i = 0; i < nF; ++i) big = fmax(big, fabs(w.A[i * ld + nF]));
          const double sc = lim / big;
          double lhs = 0.0, rhs = 0.0, num = 0.0, den = 0.0;
          for (int i = 0; i < nF; ++i) {
            double d = w.A[i * ld + nF];
            if (big > lim) d = d * sc;
            w.A[i * ld + nF] = d;
            const double xlim = w.fp[i] - 0.62 * w.fdXl[i];
            lhs += (w.fp[i] + d) * w.fdXl[i];
            rhs += xlim * w.fdXl[i];
            num += (xlim - w.fp[i]) * w.fdXl[i];
            den += d * w.fdXl[i];
          }
          const bool cross = lhs < rhs;
          const double alpha = num / den;
          bool small = true;
          for (int i = 0; i < nF; ++i) {
            if (cross) w.A[i * ld + nF] = alpha * w.A[i * ld + nF];
            small = small && fabs(w.A[i * ld + nF]) < S.free_tol;
          }
          if (small) {
            flag = 0.0;   // converged: the step is not applied
          } else {
            for (int i = 0; i < nF; ++i) {
              w.fdXl[i] = w.A[i * ld + nF];
              w.fp[i] = w.fp[i] + w.A[i * ld + nF];
            }
          }
        }
      }
      w.flag[0] = flag;
      w.flag[1] = stat;
    }
    ex.sync();
    if (go) {
      const int s2 = (int)w.flag[1];
      st = s2 > st ? s2 : st;
      go = w.flag[0] != 0.0;
    }
  }
  arr_solve_lines(S, ex, w, fr, false);   // eval_func(X) at the returned point
  if (fr) nev += 1;
  ex.sync();
}

// out[6 x nc] (row stride ld, at dst) += [I; H(r)'] M with M 3 x nc given by get(i, j)
// H(r) = get_h(r) = [[0, rz, -ry], [-rz, 0, rx], [ry, -rx, 0]]
RH_HD inline void arr_hmat(const double* r, double* H) {
  H[0] = 0.0, H[1] = r[2], H[2] = -r[1];
  H[3] = -r[2], H[4] = 0.0, H[5] = r[0];
  H[6] = r[1], H[7] = -r[0], H[8] = 0.0;
}

// dst (6 x 6 block at row 6 a, column 6 b of the nD x nD matrix K) += Ta' (sgn Ku or sgn Ku') Tb
// with Ta = [I, H(ra)], Tb = [I, H(rb)]
RH_HD inline void arr_add66(double* K, int nD, int a, int b, const double* Ku, double sgn, bool tr, const double* ra,
                            const double* rb) {
  RH_MOOR_NOFMA
  double M[9], Ha[9], Hb[9], MH[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = sgn * (tr ? Ku[3 * j + i] : Ku[3 * i + j]);
  arr_hmat(ra, Ha);
  arr_hmat(rb, Hb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) MH[3 * i + j] = M[3 * i] * Hb[j] + M[3 * i + 1] * Hb[3 + j] + M[3 * i + 2] * Hb[6 + j];
  double* d = K + (6 * a) * nD + 6 * b;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      d[i * nD + j] += M[3 * i + j];
      d[i * nD + 3 + j] += MH[3 * i + j];
      d[(3 + i) * nD + j] += Ha[i] * M[j] + Ha[3 + i] * M[3 + j] + Ha[6 + i] * M[6 + j];
      d[(3 + i) * nD + 3 + j] += Ha[i] * MH[j] + Ha[3 + i] * MH[3 + j] + Ha[6 + i] * MH[6 + j];
    }
}

// Bm (rows 6 a .. 6 a + 5, columns 3 f .. 3 f + 2 of the nD x nF matrix) += Ta' (sgn Ku or sgn Ku')
RH_HD inline void arr_add63(double* Bm, int nF, int a, int f, const double* Ku, double sgn, bool tr, const double* ra) {
  RH_MOOR_NOFMA
  double M[9], Ha[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = sgn * (tr ? Ku[3 * j + i] : Ku[3 * i + j]);
  arr_hmat(ra, Ha);
  double* d = Bm + (6 * a) * nF + 3 * f;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      d[i * nF + j] += M[3 * i + j];
      d[(3 + i) * nF + j] += Ha[i] * M[j] + Ha[3 + i] * M[3 + j] + Ha[6 + i] * M[6 + j];
    }
}

// coupled_forces(lines_only=True) into w.Fb and coupled_stiffness_analytic() into w.Kb from the
// line results of the workspace.  Leader only.  false = singular condensation matrix.
RH_HD inline bool arr_forces_stiffness(const ArrSys& S, const ArrWs& w) {
  RH_MOOR_NOFMA
  const int nD = 6 * S.nb, nF = 3 * S.nf;
  const int ld = nF + nD;
  for (int i = 0; i < nD; ++i) {
    w.Fb[i] = 0.0;
    for (int j = 0; j < nD; ++j) w.Kb[i * nD + j] = 0.0;
    for (int j = 0; j < nF; ++j) w.Bm[i * nF + j] = 0.0;
  }
  for (int i = 0; i < nF; ++i)
    for (int j = 0; j < nF; ++j) w.A[i * ld + j] = 0.0;
  for (int l = 0; l < S.nl; ++l) {
    int kA, jA, kB, jB;
    arr_line_ends(S, l, kA, jA, kB, jB);
    const double* o = w.lo + kLo * l;
    const double* Ku = o + 6;
    for (int e = 0; e < 2; ++e) {   // an end on a body: its force, moment, own stiffness and geometric term
      const int k = e ? kB : kA, b = e ? jB : jA;
      if (k != kOnBody) continue;
      const double* f = o + 3 * e;
      const double* r = o + 15 + 3 * e;
      double* F = w.Fb + 6 * b;
      F[0] += f[0], F[1] += f[1], F[2] += f[2];
      F[3] += r[1] * f[2] - r[2] * f[1];
      F[4] += r[2] * f[0] - r[0] * f[2];
      F[5] += r[0] * f[1] - r[1] * f[0];
      arr_add66(w.Kb, nD, b, b, Ku, 1.0, false, r, r);
      double Hf[9], Hr[9];
      arr_hmat(f, Hf);
      arr_hmat(r, Hr);
      double* d = w.Kb + (6 * b + 3) * nD + 6 * b + 3;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) d[i * nD + j] += -(Hf[3 * i] * Hr[j] + Hf[3 * i + 1] * Hr[3 + j] + Hf[3 * i + 2] * Hr[6 + j]);
    }
    if (kA == kOnBody && kB == kOnBody) {
      arr_add66(w.Kb, nD, jA, jB, Ku, -1.0, false, o + 15, o + 18);
      arr_add66(w.Kb, nD, jB, jA, Ku, -1.0, true, o + 18, o + 15);
    }
    if (kA == kOnBody && kB == kFree) arr_add63(w.Bm, nF, jA, jB, Ku, -1.0, false, o + 15);
    if (kB == kOnBody && kA == kFree) arr_add63(w.Bm, nF, jB, jA, Ku, -1.0, true, o + 18);
    if (kA == kFree) arr_add33(w.A, ld, jA, jA, Ku, 1.0, false);
    if (kB == kFree) arr_add33(w.A, ld, jB, jB, Ku, 1.0, false);
    if (kA == kFree && kB == kFree) {
      arr_add33(w.A, ld, jA, jB, Ku, -1.0, false);
      arr_add33(w.A, ld, jB, jA, Ku, -1.0, true);
    }
  }
  if (nF == 0) return true;
  // Kaa - Kaf Kff^-1 Kaf' carried to the body DOFs: Kb -= Bm solve(Kff, Bm')
  for (int i = 0; i < nF; ++i)
    for (int j = 0; j < nD; ++j) w.A[i * ld + nF + j] = w.Bm[j * nF + i];
  const bool ok = arr_lu_solve(w.A, nF, nD, ld);
  for (int i = 0; i < nD; ++i)
    for (int j = 0; j < nD; ++j) {
      double v = 0.0;
      for (int k = 0; k < nF; ++k) v += w.Bm[i * nF + k] * w.A[k * ld + nF + j];
      w.Kb[i * nD + j] -= v;
    }
  return ok;
}

// The largest line status of the pose so far, with `st`.  Leader only.
RH_HD inline int arr_line_status(const ArrSys& S, const ArrWs& w, int st) {
  for (int l = 0; l < S.nl; ++l) st = (int)w.lst[l] > st ? (int)w.lst[l] : st;
  return st;
}

// set_body_positions + coupled_forces + coupled_stiffness_analytic at the workspace's poses.
// Returns the pose's status (the same value in every lane of the pose).
template <class Ex>
RH_HD inline int arr_eval(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, int& nev) {
  int st = kOk;
  arr_equilibrium(S, ex, w, live, nev, st);
  if (ex.leader && live) {
    if (!arr_forces_stiffness(S, w)) st = st > kFreeSingular ? st : (int)kFreeSingular;
    w.flag[1] = (double)arr_line_status(S, w, st);
  }
  ex.sync();
  if (live) st = (int)w.flag[1];
  ex.sync();
  return live ? st : (int)kOk;
}

// Model.solveStatics (statics_mod 0, forcing_mod 0) for nb FOWTs on the record, dsolve2(a_max = 1.6,
// maxIter = 20): see statics_newton of rh_moor.h for the single-body form.  K_hs [nb][36], F_const
// [nb][6], X_ref [6 nb].  The solution stays in w.X; `iters` = evaluations (len(Model.Xs2)).
template <class Ex>
RH_HD inline void arr_statics_newton(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, const double* X_ref,
                                     const double* K_hs, const double* F_const, int& iters, int& status, int& nev) {
  RH_MOOR_NOFMA
  const int nD = 6 * S.nb;
  const int ld = nD + 1;
  if (ex.leader)
    for (int i = 0; i < nD; ++i) {
      w.X[i] = X_ref[i];
      w.dXl[i] = 0.0;
    }
  ex.sync();
  iters = 0;
  status = live ? (int)kNewtonNotConverged : (int)kOk;
  for (int it = 0; it < kNewtonMaxIter && RH_MOOR_ANY(live); ++it) {
    const int st = arr_eval(S, ex, w, live, nev);
    if (live) {
      iters += 1;
      if (st != kOk) {
        status = st;
        live = false;
      } else if (it == kNewtonMaxIter - 1) {
        live = false;
      }
    }
    if (ex.leader && live) {
      double flag = 1.0, stat = (double)kNewtonNotConverged;
      for (int b = 0; b < S.nb; ++b)
        for (int i = 0; i < 6; ++i) {
          double kx = 0.0;
          for (int j = 0; j < 6; ++j) kx += K_hs[36 * b + 6 * i + j] * (w.X[6 * b + j] - X_ref[6 * b + j]);
          w.Y[6 * b + i] = F_const[6 * b + i] + (-kx) + w.Fb[6 * b + i];
          for (int j = 0; j < 6; ++j) w.Kb[(6 * b + i) * nD + 6 * b + j] += K_hs[36 * b + 6 * i + j];
        }
      double ksum = 0.0;
      for (int i = 0; i < nD; ++i) ksum += w.Kb[i * nD + i];
      const double kmean = ksum / nD;
      for (int i = 0; i < nD; ++i)
        if (w.Kb[i * nD + i] == 0.0) w.Kb[i * nD + i] = kmean;
      bool ok = true;
      for (int r = 0; r <= 10; ++r) {   // the step, then at most ten 10 % diagonal strengthenings
        for (int i = 0; i < nD; ++i) {
          for (int j = 0; j < nD; ++j) w.A[i * ld + j] = w.Kb[i * nD + j];
          w.A[i * ld + nD] = w.Y[i];
        }
        ok = arr_lu_solve(w.A, nD, 1, ld);
        double dot = 0.0;
        for (int i = 0; i < nD; ++i) {
          w.dX[i] = w.A[i * ld + nD];
          dot += w.dX[i] * w.Y[i];
        }
        if (!ok || !(dot < 0.0) || r == 10) break;
        for (int i = 0; i < nD; ++i) w.Kb[i * nD + i] += 0.1 * fabs(w.Kb[i * nD + i]);
      }
      if (!ok) {
        flag = 0.0;
        stat = (double)kSingular;
      } else {
        double lhs = 0.0, rhs = 0.0, num = 0.0, den = 0.0;
        for (int i = 0; i < nD; ++i) {
          const double xlim = w.X[i] - 0.62 * w.dXl[i];
          lhs += (w.X[i] + w.dX[i]) * w.dXl[i];
          rhs += xlim * w.dXl[i];
          num += (xlim - w.X[i]) * w.dXl[i];
          den += w.dX[i] * w.dXl[i];
        }
        if (lhs < rhs) {
          const double alpha = num / den;
          for (int i = 0; i < nD; ++i) w.dX[i] = alpha * w.dX[i];
        }
        bool small = true;
        for (int i = 0; i < nD; ++i) small = small && fabs(w.dX[i]) < (i % 6 < 3 ? 0.05 : 0.005);
        if (small) {   // converged: the step is not applied
          flag = 0.0;
          stat = (double)kOk;
        } else {
          for (int i = 0; i < nD; ++i) {
            w.dXl[i] = w.dX[i];
            w.X[i] = w.X[i] + w.dX[i];
          }
        }
      }
      w.flag[0] = flag;
      w.flag[1] = stat;
    }
    ex.sync();
    if (live && w.flag[0] == 0.0) {
      status = (int)w.flag[1];
      live = false;
    }
    ex.sync();
  }
}

// Load a pose's state into its workspace.  Strided work (ex.sbeg, ex.sstep) is shared by the
// lanes of the pose.  pose [6 nb], warm0 [nlm][2] or null (cold), free0 [nfm][3].
template <class Ex>
RH_HD inline void arr_load_state(const ArrSys& S, const Ex& ex, const ArrWs& w, const double* pose, const double* warm0,
                                 const double* free0) {
  for (int i = ex.sbeg; i < 6 * S.nb; i += ex.sstep) w.X[i] = pose[i];
  for (int i = ex.sbeg; i < 3 * S.nf; i += ex.sstep) w.fp[i] = free0[i];
  for (int l = ex.sbeg; l < S.nl; l += ex.sstep) {
    w.wHF[l] = warm0 ? warm0[2 * l] : 0.0;
    w.wVF[l] = warm0 ? warm0[2 * l + 1] : 0.0;
    w.TA[l] = w.TB[l] = 0.0;
    w.lst[l] = 0.0;
    for (int i = 0; i < kLo; ++i) w.lo[kLo * l + i] = 0.0;
  }
  if (ex.leader) w.flag[0] = w.flag[1] = w.flag[2] = w.flag[3] = 0.0;
  ex.sync();
}

// warm [nlm][2] and free [nfm][3] of a pose from its workspace; entries the record lacks are zero
template <class Ex>
RH_HD inline void arr_store_state(const ArrSys& S, const Ex& ex, const ArrWs& w, bool write, int nlm, int nfm, double* warm,
                                  double* fre) {
  if (write) {
    for (int l = ex.sbeg; l < nlm; l += ex.sstep) {
      warm[2 * l] = l < S.nl ? w.wHF[l] : 0.0;
      warm[2 * l + 1] = l < S.nl ? w.wVF[l] : 0.0;
    }
    for (int i = ex.sbeg; i < 3 * nfm; i += ex.sstep) fre[i] = i < 3 * S.nf ? w.fp[i] : 0.0;
  }
}

// rh_moor_array_eval of one pose: F [nDm], K [nDm][nDm], T [2 nlm] (TA of line l at l, TB at nlm + l),
// J [2 nlm][nDm] or null (launch-wide), nev (line passes of the pose's own equilibrium), status.
// nDm, nlm, nfm are the call's largest 6 nb, nline and nfree (the output strides).  `live` = false
// poses (padding, a bad system index) only keep the wave company and store nothing but status.
template <class Ex>
RH_HD inline void arr_eval_pose(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, bool write, int bad_status,
                                int nDm, int nlm, int nfm, const double* pose, double* warm, double* fre, double* F,
                                double* K, double* T, double* J, int* nev_out, int* status) {
  RH_MOOR_NOFMA
  const int nD = 6 * S.nb;
  arr_load_state(S, ex, w, pose, warm, fre);
  int nev = 0;
  int st = arr_eval(S, ex, w, live, nev);
  if (write && live) {
    for (int i = ex.sbeg; i < nDm; i += ex.sstep) F[i] = i < nD ? w.Fb[i] : 0.0;
    for (int i = ex.sbeg; i < nDm * nDm; i += ex.sstep) {
      const int r = i / nDm, c = i - r * nDm;
      K[i] = (r < nD && c < nD) ? w.Kb[r * nD + c] : 0.0;
    }
    for (int l = ex.sbeg; l < nlm; l += ex.sstep) {
      T[l] = l < S.nl ? w.TA[l] : 0.0;
      T[nlm + l] = l < S.nl ? w.TB[l] : 0.0;
    }
  }
  arr_store_state(S, ex, w, write && live, nlm, nfm, warm, fre);
  if (J) {   // 0.1 m / 0.1 rad central differences, every perturbed equilibrium from the pose's own state
    const double h = 0.1;
    for (int l = ex.sbeg; l < S.nl; l += ex.sstep) w.w0HF[l] = w.wHF[l], w.w0VF[l] = w.wVF[l];
    for (int i = ex.sbeg; i < 3 * S.nf; i += ex.sstep) w.fp0[i] = w.fp[i];
    ex.sync();
    int stJ = kOk, nevJ = 0;
    for (int i = 0; i < nDm; ++i) {
      const bool li = live && i < nD;
      for (int sgn = 0; sgn < 2; ++sgn) {
        if (li) {
          if (ex.leader) w.X[i] = pose[i] + (sgn ? -h : h);
          for (int l = ex.sbeg; l < S.nl; l += ex.sstep) w.wHF[l] = w.w0HF[l], w.wVF[l] = w.w0VF[l];
          for (int k = ex.sbeg; k < 3 * S.nf; k += ex.sstep) w.fp[k] = w.fp0[k];
        }
        ex.sync();
        arr_equilibrium(S, ex, w, li, nevJ, stJ);
        if (li && sgn == 0)
          for (int l = ex.sbeg; l < S.nl; l += ex.sstep) w.TpA[l] = w.TA[l], w.TpB[l] = w.TB[l];
        if (li && sgn == 1 && ex.leader) w.X[i] = pose[i];
        ex.sync();
      }
      if (write && live)
        for (int l = ex.sbeg; l < nlm; l += ex.sstep) {
          const bool has = li && l < S.nl;
          J[l * nDm + i] = has ? (w.TpA[l] - w.TA[l]) / (2 * h) : 0.0;
          J[(nlm + l) * nDm + i] = has ? (w.TpB[l] - w.TB[l]) / (2 * h) : 0.0;
        }
      ex.sync();
    }
    if (ex.leader && live) w.flag[1] = (double)arr_line_status(S, w, st > stJ ? st : stJ);
    ex.sync();
    if (live) st = (int)w.flag[1];
  }
  if (write && ex.leader) {
    status[0] = live ? st : bad_status;
    if (nev_out) nev_out[0] = live ? nev : 0;
  }
}

// rh_array_statics_solve of one case.  X_ref [6 nb], K_hs [nb][36], F_const [nb][6]; out X [nDm].
template <class Ex>
RH_HD inline void arr_statics_case(const ArrSys& S, const Ex& ex, const ArrWs& w, bool live, bool write, int bad_status,
                                   int nDm, int nlm, int nfm, const double* X_ref, const double* K_hs,
                                   const double* F_const, const double* warm0, const double* free0, double* X, double* warm,
                                   double* fre, int* iters, int* status) {
  arr_load_state(S, ex, w, X_ref, warm0, free0);
  int it = 0, st = kOk, nev = 0;
  arr_statics_newton(S, ex, w, live, X_ref, K_hs, F_const, it, st, nev);
  if (write && live)
    for (int i = ex.sbeg; i < nDm; i += ex.sstep) X[i] = i < 6 * S.nb ? w.X[i] : 0.0;
  arr_store_state(S, ex, w, write && live, nlm, nfm, warm, fre);
  if (write && ex.leader) {
    iters[0] = live ? it : 0;
    status[0] = live ? st : bad_status;
  }
}

}  // namespace moor
}  // namespace rh
