// rh_moor_current.hip -- a translation unit of librafthip.so for two kernels: the quasi-static
// mooring evaluation and the mean-offset Newton with a uniform current on the lines
// (k_moor_eval_current, k_statics_solve_current), and their host-side launchers, which the ABI
// calls rh_moor_eval_current / rh_statics_solve_current in rh_abi.hip's unit use.
//
// The two kernels are k_moor_eval and k_statics_solve (rh_moor.hip: the mapping, the lock step and
// the shuffles are described there) with three differences: a lane also holds its line type's drag
// (4 doubles) and its pose's current (3); every line solve is moor::line_solve_current, which keeps
// the load frame's 3 x 3 rotation across the catenary loop; and so the central differences of the
// tension Jacobian re-evaluate the drag on each perturbed chord.  A pose whose current is exactly
// zero gets the bits of the kernels without current (line_solve_current's selects).
//
// They are siblings in a unit of their own, not instantiations of a body shared with the kernels
// without current, so that those keep their instructions (rh_moor.hip's header comment).  The
// lane record, its set-up and the group sums are rh_moor.hip's.  Default flags.
#define RH_MOOR_CURRENT_UNIT
#include "rh_moor.hip"

namespace rh {

// MoorLane with the current: the evaluator of moor::statics_newton in the case's current
struct MoorLaneCurrent : MoorLane {
  moor::LineCur cu;   // the line type's drag and the pose's current

  __device__ int operator()(const double* X, double* F, double* K) {
    moor::LineSol s;
    int branch;
    moor::line_solve_current(ln, cu, run, X, depth, tol, HF, VF, s, branch);
    if (run) {
      HF = s.HF;
      VF = s.VF;
    }
    TA = s.TA;
    TB = s.TB;
    status = s.status > status ? s.status : status;
    double f[6], k[36];
    moor::line_force6(s, f);
    moor::line_stiffness36(s, k);
#pragma unroll
    for (int i = 0; i < 6; ++i) F[i] = moor_group_sum(f[i], gw);
#pragma unroll
    for (int i = 0; i < 36; ++i) K[i] = moor_group_sum(k[i], gw);
    return moor_group_max(s.status, gw);
  }
};

// moor_lane_setup, then the drag of the lane's line type from drag [nsys][RH_MD_COUNT][nl_max] and
// the pose's current from current [npose][3].  Padding lanes read the columns of the line they
// were given (in bounds); a pose with a bad system index reads system 0's and idles.
__device__ __forceinline__ bool moor_lane_setup_current(const rh_moor_system* __restrict__ sys, int nsys,
                                                        const int* __restrict__ sys_idx, int pose, int l, bool pose_ok,
                                                        int gw, int nl_max, const double* __restrict__ drag,
                                                        const double* __restrict__ current, MoorLaneCurrent& L) {
  const bool sys_ok = moor_lane_setup(sys, nsys, sys_idx, pose, l, pose_ok, gw, L);
  const int si = sys_ok && sys_idx ? sys_idx[pose] : 0;
  const int n = sys[si].nline;
  const int ll = l < n ? l : n - 1;
  const double* __restrict__ t = drag + (size_t)si * RH_MD_COUNT * nl_max;
  L.cu.d = t[RH_MD_D * nl_max + ll];
  L.cu.Cd = t[RH_MD_CD * nl_max + ll];
  L.cu.CdAx = t[RH_MD_CDAX * nl_max + ll];
  L.cu.rho = t[RH_MD_RHO * nl_max + ll];
  L.cu.Ux = current[(size_t)pose * 3];
  L.cu.Uy = current[(size_t)pose * 3 + 1];
  L.cu.Uz = current[(size_t)pose * 3 + 2];
  return sys_ok;
}

// grid ceil(npose gw / 256), 256 threads
__global__ __launch_bounds__(256) void k_moor_eval_current(const rh_moor_system* __restrict__ sys, int nsys, int npose,
                                                           int gw, int nl_max, const int* __restrict__ sys_idx,
                                                           const double* __restrict__ r6,
                                                           const double* __restrict__ drag,
                                                           const double* __restrict__ current,
                                                           double* __restrict__ warm, double* __restrict__ F,
                                                           double* __restrict__ K, double* __restrict__ T,
                                                           double* __restrict__ J, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int pose_raw = t / gw;
  const int l = t - pose_raw * gw;
  const bool pose_ok = pose_raw < npose;
  const int pose = pose_ok ? pose_raw : npose - 1;   // lanes past the end load the last pose and store nothing
  MoorLaneCurrent L;
  const bool sys_ok = moor_lane_setup_current(sys, nsys, sys_idx, pose, l, pose_ok, gw, nl_max, drag, current, L);
  const bool mine = pose_ok && l < nl_max;           // this lane owns a column of warm / T / J
  double X[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) X[i] = r6[(size_t)pose * 6 + i];
  if (warm && l < nl_max) {
    L.HF = warm[((size_t)pose * nl_max + l) * 2];
    L.VF = warm[((size_t)pose * nl_max + l) * 2 + 1];
  }
  double Fs[6], Ks[36];
  int st = L(X, Fs, Ks);
  if (pose_ok && l == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) F[(size_t)pose * 6 + i] = Fs[i];
#pragma unroll
    for (int i = 0; i < 36; ++i) K[(size_t)pose * 36 + i] = Ks[i];
  }
  if (mine) {
    T[(size_t)pose * 2 * nl_max + l] = L.TA;
    T[(size_t)pose * 2 * nl_max + nl_max + l] = L.TB;
    if (warm) {
      warm[((size_t)pose * nl_max + l) * 2] = L.run ? L.HF : 0.0;
      warm[((size_t)pose * nl_max + l) * 2 + 1] = L.run ? L.VF : 0.0;
    }
  }
  if (J) {   // central differences, every perturbed solve from the pose's own solution, the drag on its own chord
    const double HFb = L.HF, VFb = L.VF;
    for (int i = 0; i < 6; ++i) {
      const double h = 0.1;   // dx = dth = 0.1
      double Xp[6], Xm[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        Xp[j] = X[j] + (j == i ? h : 0.0);
        Xm[j] = X[j] + (j == i ? -h : 0.0);
      }
      moor::LineSol sp, sm;
      int branch;
      moor::line_solve_current(L.ln, L.cu, L.run, Xp, L.depth, L.tol, HFb, VFb, sp, branch);
      moor::line_solve_current(L.ln, L.cu, L.run, Xm, L.depth, L.tol, HFb, VFb, sm, branch);
      const int sw = sp.status > sm.status ? sp.status : sm.status;
      L.status = sw > L.status ? sw : L.status;
      if (mine) {
        J[((size_t)pose * 2 * nl_max + l) * 6 + i] = (sp.TA - sm.TA) / (2 * h);
        J[((size_t)pose * 2 * nl_max + nl_max + l) * 6 + i] = (sp.TB - sm.TB) / (2 * h);
      }
    }
    st = moor_group_max(L.status, gw);
  }
  if (pose_ok && l == 0) status[pose] = sys_ok ? st : (int)moor::kBadSystem;
}

// grid ceil(ncase gw / 256), 256 threads
__global__ __launch_bounds__(256) void k_statics_solve_current(
    const rh_moor_system* __restrict__ sys, int nsys, int ncase, int gw, int nl_max, const int* __restrict__ sys_idx,
    const double* __restrict__ X_ref, const double* __restrict__ K_hs, const double* __restrict__ F_const,
    const double* __restrict__ drag, const double* __restrict__ current, const double* __restrict__ warm0,
    double* __restrict__ Xout, double* __restrict__ warm, int* __restrict__ iters, int* __restrict__ status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int case_raw = t / gw;
  const int l = t - case_raw * gw;
  const bool case_ok = case_raw < ncase;
  const int c = case_ok ? case_raw : ncase - 1;
  MoorLaneCurrent L;
  const bool sys_ok = moor_lane_setup_current(sys, nsys, sys_idx, c, l, case_ok, gw, nl_max, drag, current, L);
  if (warm0 && l < nl_max) {
    L.HF = warm0[((size_t)c * nl_max + l) * 2];
    L.VF = warm0[((size_t)c * nl_max + l) * 2 + 1];
  }
  double X[6];
  int it, st;
  // K_hs, X_ref and F_const stay in memory, as in k_statics_solve
  moor::statics_newton(L, case_ok && sys_ok, X_ref + (size_t)c * 6, K_hs + (size_t)c * 36, F_const + (size_t)c * 6, X, it,
                       st);
  if (case_ok && l == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) Xout[(size_t)c * 6 + i] = X[i];
    iters[c] = it;
    status[c] = sys_ok ? st : (int)moor::kBadSystem;
  }
  if (case_ok && l < nl_max) {
    warm[((size_t)c * nl_max + l) * 2] = L.run ? L.HF : 0.0;
    warm[((size_t)c * nl_max + l) * 2 + 1] = L.run ? L.VF : 0.0;
  }
}

hipError_t launch_moor_eval_current(dim3 grid, hipStream_t s, const rh_moor_system* sys, int nsys, int npose, int gw,
                                    int nl_max, const int* sys_idx, const double* r6, const double* drag,
                                    const double* current, double* warm, double* F, double* K, double* T, double* J,
                                    int* status) {
  hipLaunchKernelGGL(k_moor_eval_current, grid, dim3(256), 0, s, sys, nsys, npose, gw, nl_max, sys_idx, r6, drag, current,
                     warm, F, K, T, J, status);
  return hipGetLastError();
}

hipError_t launch_statics_solve_current(dim3 grid, hipStream_t s, const rh_moor_system* sys, int nsys, int ncase, int gw,
                                        int nl_max, const int* sys_idx, const double* X_ref, const double* K_hs,
                                        const double* F_const, const double* drag, const double* current,
                                        const double* warm0, double* X, double* warm, int* iters, int* status) {
  hipLaunchKernelGGL(k_statics_solve_current, grid, dim3(256), 0, s, sys, nsys, ncase, gw, nl_max, sys_idx, X_ref, K_hs,
                     F_const, drag, current, warm0, X, warm, iters, status);
  return hipGetLastError();
}

}  // namespace rh
