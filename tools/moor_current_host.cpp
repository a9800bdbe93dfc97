// Host build of rh_moor.h's current branch for the CPU check against raft/mooring.py
// (Line.static_solve(current=U), MooringSystem with .current set) and Model.solveStatics on a
// mooring currentMod 1 design (tests/test_moor_current_host.py): the line solve, the evaluation
// and the Newton the device runs in rh_moor_eval_current / rh_statics_solve_current, with the
// per-case sums taken line after line instead of across lanes.
#include "../raft-teststuff_amd/csrc/rh_moor.h"
#include "../include/rafthip.h"

namespace {

rh::moor::LineIn load_line(const double* t, int n, int l) {
  rh::moor::LineIn ln;
  ln.fx = t[RH_ML_FX * n + l], ln.fy = t[RH_ML_FY * n + l], ln.fz = t[RH_ML_FZ * n + l];
  ln.ax = t[RH_ML_AX * n + l], ln.ay = t[RH_ML_AY * n + l], ln.az = t[RH_ML_AZ * n + l];
  ln.L = t[RH_ML_L * n + l], ln.EA = t[RH_ML_EA * n + l], ln.W = t[RH_ML_W * n + l];
  ln.att_end = t[RH_ML_END * n + l] != 0.0 ? 1 : 0;
  return ln;
}

// drag [RH_MD_COUNT][n] of one system, U [3]
rh::moor::LineCur load_current(const double* drag, int n, int l, const double* U) {
  rh::moor::LineCur cu;
  cu.d = drag[RH_MD_D * n + l], cu.Cd = drag[RH_MD_CD * n + l], cu.CdAx = drag[RH_MD_CDAX * n + l];
  cu.rho = drag[RH_MD_RHO * n + l];
  cu.Ux = U[0], cu.Uy = U[1], cu.Uz = U[2];
  return cu;
}

// the evaluator of rh::moor::statics_newton on the host: every line in turn, in the current U
struct HostEvalCurrent {
  int n;
  double depth, tol;
  const double* table;
  const double* drag;
  const double* U;
  double* warm;   // [n][2] in/out
  double* T;      // [2 n] or null
  int operator()(const double* X, double* F, double* K) {
    int st = 0;
    for (int i = 0; i < 6; ++i) F[i] = 0.0;
    for (int i = 0; i < 36; ++i) K[i] = 0.0;
    for (int l = 0; l < n; ++l) {
      rh::moor::LineSol s;
      int branch;
      rh::moor::line_solve_current(load_line(table, n, l), load_current(drag, n, l, U), true, X, depth, tol,
                                   warm[2 * l], warm[2 * l + 1], s, branch);
      warm[2 * l] = s.HF, warm[2 * l + 1] = s.VF;
      if (T) T[l] = s.TA, T[n + l] = s.TB;
      double f[6], k[36];
      rh::moor::line_force6(s, f);
      rh::moor::line_stiffness36(s, k);
      for (int i = 0; i < 6; ++i) F[i] += f[i];
      for (int i = 0; i < 36; ++i) K[i] += k[i];
      st = s.status > st ? s.status : st;
    }
    return st;
  }
};

}  // namespace

// One line (row 0 of a one-line table and drag table) at body pose r6 in the current U, from the
// warm start (HF0, VF0).  out [20]: force on the attached point (3), Ku (9), TA, TB, HF, VF,
// residual evaluations, status, branch (bit 0: current branch taken, bit 1: the load points up),
// and 0.  plain != 0 calls line_solve (no current) instead: the bits U = 0 has to reproduce.
extern "C" void rh_moor_line_current_host(const double* table, const double* drag, const double* U, const double* r6,
                                          double depth, double tol, double HF0, double VF0, int plain, double* out) {
  rh::moor::LineSol s;
  int branch = 0;
  const rh::moor::LineIn ln = load_line(table, 1, 0);
  if (plain) rh::moor::line_solve(ln, true, r6, depth, tol, HF0, VF0, s);
  else rh::moor::line_solve_current(ln, load_current(drag, 1, 0, U), true, r6, depth, tol, HF0, VF0, s, branch);
  out[0] = s.fx, out[1] = s.fy, out[2] = s.fz;
  for (int i = 0; i < 9; ++i) out[3 + i] = s.Ku[i];
  out[12] = s.TA, out[13] = s.TB, out[14] = s.HF, out[15] = s.VF;
  out[16] = s.iters, out[17] = s.status, out[18] = branch, out[19] = 0.0;
}

// rh_moor_eval_current of one system at npose poses, current [npose][3]; T, J rows as [TA_1..TA_n, TB_1..TB_n]
extern "C" void rh_moor_eval_current_host(int nline, double depth, double tol, const double* table, const double* drag,
                                          int npose, const double* r6, const double* current, double* warm, double* F,
                                          double* K, double* T, double* J, int* status) {
  for (int p = 0; p < npose; ++p) {
    const double* U = current + (long)p * 3;
    HostEvalCurrent ev{nline, depth, tol, table, drag, U, warm + (long)p * nline * 2, T + (long)p * 2 * nline};
    const double* X = r6 + (long)p * 6;
    int st = ev(X, F + (long)p * 6, K + (long)p * 36);
    if (J) {
      for (int i = 0; i < 6; ++i) {
        const double h = 0.1;
        double Xp[6], Xm[6];
        for (int j = 0; j < 6; ++j) Xp[j] = X[j] + (j == i ? h : 0.0), Xm[j] = X[j] + (j == i ? -h : 0.0);
        for (int l = 0; l < nline; ++l) {
          rh::moor::LineSol sp, sm;
          int branch;
          const rh::moor::LineIn ln = load_line(table, nline, l);
          const rh::moor::LineCur cu = load_current(drag, nline, l, U);
          rh::moor::line_solve_current(ln, cu, true, Xp, depth, tol, ev.warm[2 * l], ev.warm[2 * l + 1], sp, branch);
          rh::moor::line_solve_current(ln, cu, true, Xm, depth, tol, ev.warm[2 * l], ev.warm[2 * l + 1], sm, branch);
          J[((long)p * 2 * nline + l) * 6 + i] = (sp.TA - sm.TA) / (2 * h);
          J[((long)p * 2 * nline + nline + l) * 6 + i] = (sp.TB - sm.TB) / (2 * h);
          st = sp.status > st ? sp.status : st;
          st = sm.status > st ? sm.status : st;
        }
      }
    }
    status[p] = st;
  }
}

// rh_statics_solve_current of one case in the current U [3]
extern "C" void rh_statics_solve_current_host(int nline, double depth, double tol, const double* table,
                                              const double* drag, const double* U, const double* X_ref,
                                              const double* K_hs, const double* F_const, const double* warm0, double* X,
                                              double* warm, int* iters, int* status) {
  for (int i = 0; i < 2 * nline; ++i) warm[i] = warm0 ? warm0[i] : 0.0;
  HostEvalCurrent ev{nline, depth, tol, table, drag, U, warm, nullptr};
  rh::moor::statics_newton(ev, true, X_ref, K_hs, F_const, X, *iters, *status);
}
