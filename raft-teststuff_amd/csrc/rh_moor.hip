// rh_moor.hip -- quasi-static mooring and mean offsets on the device: the kernels over the
// host/device math of rh_moor.h, and their ABI calls (rh_moor_eval, rh_statics_solve, and the two
// with a uniform current on the lines, rh_moor_eval_current and rh_statics_solve_current).
// Included by rh_abi.hip after its `fail` / RH_HIP helpers.
//
// Mapping: one lane per (pose, line).  The lines of a pose sit in adjacent lanes of a group of
// gw = the next power of two >= the call's largest nline (gw <= 64, so a group never straddles a
// wave); lanes past a system's nline are padding and contribute zeros.  The per-pose sums (6
// forces, 36 stiffness entries) and the status go across the group with __shfl_xor butterflies,
// whose result is the same bits in every lane of the group (FP add commutes), so every lane
// then runs the same 6 x 6 Newton step and nothing is broadcast.  Catenary and Newton loops run
// to the wave's vote with finished lanes predicated off (rh_moor.h), so all 64 lanes reach every
// shuffle and a pose's numbers never depend on the poses next to it.  No LDS; FP64 VALU only;
// plain vector loads and stores.
//
// Current on the lines: k_moor_eval_current and k_statics_solve_current (rh_moor_current.hip, a
// translation unit of its own that includes this file with RH_MOOR_CURRENT_UNIT defined for the
// lane helpers) are siblings of the two kernels here.  They are siblings and not instantiations of
// shared templates, and live in another unit, because the kernels without current have to keep
// their instructions (tools/asm_same.py): a shared templated body, or the mere presence of further
// callers of rh_moor.h's inline functions in the unit, gives them another register allocation.
#pragma once
#include "rh_common.h"
#include "rh_moor.h"

namespace rh {

__device__ __forceinline__ double moor_group_sum(double v, int gw) {
  for (int m = 1; m < gw; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ int moor_group_max(int v, int gw) {
  for (int m = 1; m < gw; m <<= 1) {
    const int o = __shfl_xor(v, m);
    v = o > v ? o : v;
  }
  return v;
}

// One lane's line and the warm state it carries from one evaluation to the next.
struct MoorLane {
  moor::LineIn ln;
  double depth, tol;
  double HF, VF;     // catenary warm start of the next solve (0 = cold)
  double TA, TB;     // end tensions of the last solve
  int gw;
  int status;        // the largest line status seen so far (this lane's)
  bool run;          // this lane has a line of a valid pose

  // the evaluator of moor::statics_newton: F_moor(X), C_moor(X), status, the same in every lane
  __device__ int operator()(const double* X, double* F, double* K) {
    moor::LineSol s;
    moor::line_solve(ln, run, X, depth, tol, HF, VF, s);
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

// Fill a lane from the system table.  Returns false when the pose's system index is out of range
// (the whole group then idles).  Padding lanes get a harmless line.
__device__ __forceinline__ bool moor_lane_setup(const rh_moor_system* __restrict__ sys, int nsys,
                                                const int* __restrict__ sys_idx, int pose, int l, bool pose_ok, int gw,
                                                MoorLane& L) {
  const int si = sys_idx ? sys_idx[pose] : 0;
  const bool sys_ok = si >= 0 && si < nsys;
  const rh_moor_system S = sys[sys_ok ? si : 0];
  L.gw = gw;
  L.depth = S.depth;
  L.tol = S.tol;
  L.HF = L.VF = 0.0;
  L.TA = L.TB = 0.0;
  L.status = moor::kOk;
  L.run = pose_ok && sys_ok && l < S.nline;
  const int n = S.nline;
  const int ll = l < n ? l : n - 1;   // padding lanes read the last line (in bounds) and discard it
  const double* __restrict__ t = S.line;
  L.ln.fx = t[RH_ML_FX * n + ll];
  L.ln.fy = t[RH_ML_FY * n + ll];
  L.ln.fz = t[RH_ML_FZ * n + ll];
  L.ln.ax = t[RH_ML_AX * n + ll];
  L.ln.ay = t[RH_ML_AY * n + ll];
  L.ln.az = t[RH_ML_AZ * n + ll];
  L.ln.L = t[RH_ML_L * n + ll];
  L.ln.EA = t[RH_ML_EA * n + ll];
  L.ln.W = t[RH_ML_W * n + ll];
  L.ln.att_end = t[RH_ML_END * n + ll] != 0.0 ? 1 : 0;
  return sys_ok;
}

#ifndef RH_MOOR_CURRENT_UNIT
// grid ceil(npose gw / 256), 256 threads
__global__ __launch_bounds__(256) void k_moor_eval(const rh_moor_system* __restrict__ sys, int nsys, int npose, int gw,
                                                   int nl_max, const int* __restrict__ sys_idx,
                                                   const double* __restrict__ r6, double* __restrict__ warm,
                                                   double* __restrict__ F, double* __restrict__ K,
                                                   double* __restrict__ T, double* __restrict__ J,
                                                   int* __restrict__ status) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int pose_raw = t / gw;
  const int l = t - pose_raw * gw;
  const bool pose_ok = pose_raw < npose;
  const int pose = pose_ok ? pose_raw : npose - 1;   // lanes past the end load the last pose and store nothing
  MoorLane L;
  const bool sys_ok = moor_lane_setup(sys, nsys, sys_idx, pose, l, pose_ok, gw, L);
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
  if (J) {   // central differences, every perturbed solve from the pose's own solution
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
      moor::line_solve(L.ln, L.run, Xp, L.depth, L.tol, HFb, VFb, sp);
      moor::line_solve(L.ln, L.run, Xm, L.depth, L.tol, HFb, VFb, sm);
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
__global__ __launch_bounds__(256) void k_statics_solve(const rh_moor_system* __restrict__ sys, int nsys, int ncase,
                                                       int gw, int nl_max, const int* __restrict__ sys_idx,
                                                       const double* __restrict__ X_ref,
                                                       const double* __restrict__ K_hs,
                                                       const double* __restrict__ F_const,
                                                       const double* __restrict__ warm0, double* __restrict__ Xout,
                                                       double* __restrict__ warm, int* __restrict__ iters,
                                                       int* __restrict__ status) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int case_raw = t / gw;
  const int l = t - case_raw * gw;
  const bool case_ok = case_raw < ncase;
  const int c = case_ok ? case_raw : ncase - 1;
  MoorLane L;
  const bool sys_ok = moor_lane_setup(sys, nsys, sys_idx, c, l, case_ok, gw, L);
  if (warm0 && l < nl_max) {
    L.HF = warm0[((size_t)c * nl_max + l) * 2];
    L.VF = warm0[((size_t)c * nl_max + l) * 2 + 1];
  }
  double X[6];
  int it, st;
  // K_hs, X_ref and F_const stay in memory (36 + 12 doubles a lane would otherwise hold in VGPRs
  // across the whole iteration); every lane of a group reads the same cached addresses
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

// (defined in rh_moor_current.hip)
hipError_t launch_moor_eval_current(dim3 grid, hipStream_t s, const rh_moor_system* sys, int nsys, int npose, int gw,
                                    int nl_max, const int* sys_idx, const double* r6, const double* drag,
                                    const double* current, double* warm, double* F, double* K, double* T, double* J,
                                    int* status);
hipError_t launch_statics_solve_current(dim3 grid, hipStream_t s, const rh_moor_system* sys, int nsys, int ncase, int gw,
                                        int nl_max, const int* sys_idx, const double* X_ref, const double* K_hs,
                                        const double* F_const, const double* drag, const double* current,
                                        const double* warm0, double* X, double* warm, int* iters, int* status);
#endif   // RH_MOOR_CURRENT_UNIT

}  // namespace rh

#ifndef RH_MOOR_CURRENT_UNIT
namespace {
// validates the host records; returns the group width through gw and the largest nline through nl_max
int check_moor_systems(const rh_moor_system* sys, const rh_moor_system* sys_dev, int nsys, int n, const char* who,
                       int& gw, int& nl_max) {
  if (!sys || !sys_dev) return fail(RH_EINVAL, "%s: null system array", who);
  if (nsys < 1) return fail(RH_EINVAL, "%s: nsys=%d must be >= 1", who, nsys);
  if (n < 0 || n > (1 << 24)) return fail(RH_EINVAL, "%s: %d poses outside [0, 2^24]", who, n);
  nl_max = 0;
  for (int i = 0; i < nsys; ++i) {
    const rh_moor_system& s = sys[i];
    if (s.nline < 1 || s.nline > RH_MOOR_MAX_LINES)
      return fail(RH_EINVAL, "%s: system %d: nline=%d outside [1, %d]", who, i, s.nline, RH_MOOR_MAX_LINES);
    if (!s.line) return fail(RH_EINVAL, "%s: system %d: null line table", who, i);
    if (!(s.tol > 0.0) || !(s.tol < 1.0)) return fail(RH_EINVAL, "%s: system %d: tol=%g outside (0, 1)", who, i, s.tol);
    if (!(s.depth == s.depth)) return fail(RH_EINVAL, "%s: system %d: depth is NaN", who, i);
    nl_max = s.nline > nl_max ? s.nline : nl_max;
  }
  gw = 1;
  while (gw < nl_max) gw <<= 1;
  return RH_OK;
}
}  // namespace

int rh_moor_eval(rh_ctx* ctx, const rh_moor_system* sys, const rh_moor_system* sys_dev, int nsys, int npose,
                 const int* sys_idx, const double* r6, double* warm, double* F, double* K, double* T, double* J,
                 int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_moor_eval: null context");
  int gw, nl_max;
  if (int r = check_moor_systems(sys, sys_dev, nsys, npose, "rh_moor_eval", gw, nl_max)) return r;
  if (npose == 0) return RH_OK;
  if (!r6 || !F || !K || !T || !status) return fail(RH_EINVAL, "rh_moor_eval: null r6, F, K, T or status");
  RH_HIP(hipSetDevice(ctx->device));
  const long long lanes = (long long)npose * gw;
  hipLaunchKernelGGL(rh::k_moor_eval, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sys_dev,
                     nsys, npose, gw, nl_max, sys_idx, r6, warm, F, K, T, J, status);
  RH_HIP(hipGetLastError());
  return RH_OK;
}

int rh_statics_solve(rh_ctx* ctx, const rh_moor_system* sys, const rh_moor_system* sys_dev, int nsys, int ncase,
                     const int* sys_idx, const double* X_ref, const double* K_hs, const double* F_const,
                     const double* warm0, double* X, double* warm, int* iters, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_statics_solve: null context");
  int gw, nl_max;
  if (int r = check_moor_systems(sys, sys_dev, nsys, ncase, "rh_statics_solve", gw, nl_max)) return r;
  if (ncase == 0) return RH_OK;
  if (!X_ref || !K_hs || !F_const || !X || !warm || !iters || !status)
    return fail(RH_EINVAL, "rh_statics_solve: null X_ref, K_hs, F_const, X, warm, iters or status");
  RH_HIP(hipSetDevice(ctx->device));
  const long long lanes = (long long)ncase * gw;
  hipLaunchKernelGGL(rh::k_statics_solve, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     sys_dev, nsys, ncase, gw, nl_max, sys_idx, X_ref, K_hs, F_const, warm0, X, warm, iters, status);
  RH_HIP(hipGetLastError());
  return RH_OK;
}

int rh_moor_eval_current(rh_ctx* ctx, const rh_moor_system* sys, const rh_moor_system* sys_dev, int nsys, int npose,
                         const int* sys_idx, const double* r6, const double* drag, const double* current,
                         double* warm, double* F, double* K, double* T, double* J, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_moor_eval_current: null context");
  int gw, nl_max;
  if (int r = check_moor_systems(sys, sys_dev, nsys, npose, "rh_moor_eval_current", gw, nl_max)) return r;
  if (!drag || !current) return fail(RH_EINVAL, "rh_moor_eval_current: null drag or current");
  if (npose == 0) return RH_OK;
  if (!r6 || !F || !K || !T || !status) return fail(RH_EINVAL, "rh_moor_eval_current: null r6, F, K, T or status");
  RH_HIP(hipSetDevice(ctx->device));
  const long long lanes = (long long)npose * gw;
  RH_HIP(rh::launch_moor_eval_current(dim3((unsigned)((lanes + 255) / 256)), (hipStream_t)stream, sys_dev, nsys, npose, gw,
                                      nl_max, sys_idx, r6, drag, current, warm, F, K, T, J, status));
  return RH_OK;
}

int rh_statics_solve_current(rh_ctx* ctx, const rh_moor_system* sys, const rh_moor_system* sys_dev, int nsys, int ncase,
                             const int* sys_idx, const double* X_ref, const double* K_hs, const double* F_const,
                             const double* drag, const double* current, const double* warm0, double* X, double* warm,
                             int* iters, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_statics_solve_current: null context");
  int gw, nl_max;
  if (int r = check_moor_systems(sys, sys_dev, nsys, ncase, "rh_statics_solve_current", gw, nl_max)) return r;
  if (!drag || !current) return fail(RH_EINVAL, "rh_statics_solve_current: null drag or current");
  if (ncase == 0) return RH_OK;
  if (!X_ref || !K_hs || !F_const || !X || !warm || !iters || !status)
    return fail(RH_EINVAL, "rh_statics_solve_current: null X_ref, K_hs, F_const, X, warm, iters or status");
  RH_HIP(hipSetDevice(ctx->device));
  const long long lanes = (long long)ncase * gw;
  RH_HIP(rh::launch_statics_solve_current(dim3((unsigned)((lanes + 255) / 256)), (hipStream_t)stream, sys_dev, nsys,
                                          ncase, gw, nl_max, sys_idx, X_ref, K_hs, F_const, drag, current, warm0, X, warm,
                                          iters, status));
  return RH_OK;
}
#endif   // RH_MOOR_CURRENT_UNIT
