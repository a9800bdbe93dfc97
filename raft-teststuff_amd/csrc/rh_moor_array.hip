// rh_moor_array.hip -- general mooring systems and the mean offsets of moored arrays on the
// device: the kernels over the host/device math of rh_moor_array.h, and their two ABI calls
// (rh_moor_array_eval, rh_array_statics_solve).  Included by rh_abi.hip after rh_moor.hip.
//
// Mapping: one lane per (pose, line), as rh_moor.hip.  The lines of a pose sit in adjacent lanes of
// a group of gw lanes (a power of two >= the call's largest nline, <= 64), and ONE wave is a
// workgroup, so the workgroup barrier between the line work and the dense work is a barrier of
// that wave alone: the catenary loop, the free-point Newton and the body Newton run to the wave's
// vote with finished poses predicated off, every lane reaches every barrier, and no second wave
// exists that could disagree on a trip count.  The dense work (free-point matrix up to 24 x 24,
// condensation, the 6nb x 6nb pivoted LU) is done by the first lane of the group on the pose's LDS
// workspace, line after line in table order: the sums of a pose have one order, whatever the launch
// size and the neighbouring poses.  gw is widened until the workspaces of a wave's 64 / gw poses fit
// in 64 KiB of LDS.  FP64 VALU only, no atomics, plain vector loads and stores.
#pragma once
#include "rh_common.h"
#include "rh_moor_array.h"

namespace rh {

constexpr size_t kMoorArrLds = 64 * 1024;

struct MoorArrEx {
  int lbeg, lend, sbeg, sstep;
  bool leader;
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

struct MoorArrLaunch {
  const rh_moor_array_system* sys;
  int nsys, n, gw, nbm, nlm, nfm, wsd;   // wsd: doubles of one pose's workspace
  const int* sys_idx;
};

// The lane's record, workspace and role.  Returns whether the pose's system index is in range.
__device__ __forceinline__ bool moor_arr_setup(const MoorArrLaunch& a, double* lds, int& pose, bool& pose_ok,
                                               moor::ArrSys& S, moor::ArrWs& w, MoorArrEx& ex) {
  const int ppb = 64 / a.gw;
  const int g = (int)threadIdx.x / a.gw;
  const int l = (int)threadIdx.x - g * a.gw;
  const int pose_raw = (int)blockIdx.x * ppb + g;
  pose_ok = pose_raw < a.n;
  pose = pose_ok ? pose_raw : a.n - 1;   // groups past the end load the last pose and store nothing
  const int si = a.sys_idx ? a.sys_idx[pose] : 0;
  const bool sys_ok = si >= 0 && si < a.nsys;
  const rh_moor_array_system R = a.sys[sys_ok ? si : 0];
  S.nb = R.nbody < a.nbm ? R.nbody : a.nbm;
  S.np = R.npoint;
  S.nl = R.nline < a.nlm ? R.nline : a.nlm;
  S.nf = R.nfree < a.nfm ? R.nfree : a.nfm;
  S.free_sys = R.free_sys;
  S.g = R.g, S.rho = R.rho, S.free_tol = R.free_tol, S.free_depth = R.free_depth;
  S.pt = R.point, S.ln = R.line;
  moor::arr_ws_carve(lds + (size_t)g * a.wsd, 6 * a.nbm, 3 * a.nfm, a.nlm, w);
  ex.lbeg = l, ex.lend = l + 1, ex.sbeg = l, ex.sstep = a.gw;
  ex.leader = l == 0;
  return sys_ok;
}

// grid ceil(npose / (64 / gw)), 64 threads, dynamic LDS (64 / gw) wsd doubles
__global__ __launch_bounds__(64) void k_moor_array_eval(MoorArrLaunch a, const double* __restrict__ r6,
                                                        double* __restrict__ warm, double* __restrict__ fre,
                                                        double* __restrict__ F, double* __restrict__ K,
                                                        double* __restrict__ T, double* __restrict__ J,
                                                        int* __restrict__ nev, int* __restrict__ status) {
  extern __shared__ double moor_arr_lds[];
  int pose;
  bool pose_ok;
  moor::ArrSys S;
  moor::ArrWs w;
  MoorArrEx ex;
  const bool sys_ok = moor_arr_setup(a, moor_arr_lds, pose, pose_ok, S, w, ex);
  const int nDm = 6 * a.nbm;
  const size_t p = (size_t)pose;
  moor::arr_eval_pose(S, ex, w, pose_ok && sys_ok, pose_ok, (int)moor::kBadSystem, nDm, a.nlm, a.nfm, r6 + p * nDm,
                      warm + p * 2 * a.nlm, fre + p * 3 * a.nfm, F + p * nDm, K + p * nDm * nDm, T + p * 2 * a.nlm,
                      J ? J + p * 2 * a.nlm * nDm : nullptr, nev ? nev + p : nullptr, status + p);
}

__global__ __launch_bounds__(64) void k_array_statics_solve(MoorArrLaunch a, const double* __restrict__ X_ref,
                                                            const double* __restrict__ K_hs,
                                                            const double* __restrict__ F_const,
                                                            const double* __restrict__ warm0,
                                                            const double* __restrict__ free0, double* __restrict__ X,
                                                            double* __restrict__ warm, double* __restrict__ fre,
                                                            int* __restrict__ iters, int* __restrict__ status) {
  extern __shared__ double moor_arr_lds[];
  int c;
  bool case_ok;
  moor::ArrSys S;
  moor::ArrWs w;
  MoorArrEx ex;
  const bool sys_ok = moor_arr_setup(a, moor_arr_lds, c, case_ok, S, w, ex);
  const int nDm = 6 * a.nbm;
  const size_t p = (size_t)c;
  moor::arr_statics_case(S, ex, w, case_ok && sys_ok, case_ok, (int)moor::kBadSystem, nDm, a.nlm, a.nfm, X_ref + p * nDm,
                         K_hs + p * 36 * a.nbm, F_const + p * nDm, warm0 ? warm0 + p * 2 * a.nlm : nullptr,
                         free0 + p * 3 * a.nfm, X + p * nDm, warm + p * 2 * a.nlm, fre + p * 3 * a.nfm, iters + p,
                         status + p);
}

}  // namespace rh

namespace {
// validates the host records and their host tables; fills the launch geometry
int check_moor_array_systems(const rh_moor_array_system* sys, const rh_moor_array_system* sys_dev, int nsys, int n,
                             const char* who, rh::MoorArrLaunch& a) {
  if (!sys || !sys_dev) return fail(RH_EINVAL, "%s: null system array", who);
  if (nsys < 1) return fail(RH_EINVAL, "%s: nsys=%d must be >= 1", who, nsys);
  if (n < 0 || n > (1 << 24)) return fail(RH_EINVAL, "%s: %d poses outside [0, 2^24]", who, n);
  a.nbm = a.nlm = a.nfm = 0;
  for (int i = 0; i < nsys; ++i) {
    const rh_moor_array_system& s = sys[i];
    if (s.nbody < 1 || s.nbody > RH_MOOR_MAX_BODIES)
      return fail(RH_EINVAL, "%s: system %d: nbody=%d outside [1, %d]", who, i, s.nbody, RH_MOOR_MAX_BODIES);
    if (s.nfree < 0 || s.nfree > RH_MOOR_MAX_FREE)
      return fail(RH_EINVAL, "%s: system %d: nfree=%d outside [0, %d]", who, i, s.nfree, RH_MOOR_MAX_FREE);
    if (s.nline < 1 || s.nline > RH_MOOR_MAX_LINES)
      return fail(RH_EINVAL, "%s: system %d: nline=%d outside [1, %d]", who, i, s.nline, RH_MOOR_MAX_LINES);
    if (s.npoint < 2 || s.npoint > 2 * RH_MOOR_MAX_LINES)
      return fail(RH_EINVAL, "%s: system %d: npoint=%d outside [2, %d]", who, i, s.npoint, 2 * RH_MOOR_MAX_LINES);
    if (!s.point || !s.line || !s.point_host || !s.line_host)
      return fail(RH_EINVAL, "%s: system %d: null point or line table", who, i);
    if (s.nfree > 0 && (!(s.free_tol > 0.0) || !(s.g == s.g) || !(s.rho == s.rho) || !(s.free_depth == s.free_depth)))
      return fail(RH_EINVAL, "%s: system %d: free_tol=%g must be > 0 and g, rho, free_depth numbers", who, i, s.free_tol);
    int nfree = 0;
    for (int p = 0; p < s.npoint; ++p) {
      const double kind = s.point_host[RH_MP_KIND * s.npoint + p], idx = s.point_host[RH_MP_INDEX * s.npoint + p];
      if (!(kind == 0.0 || kind == 1.0 || kind == 2.0))
        return fail(RH_EINVAL, "%s: system %d: point %d: kind %g (0 fixed, 1 on a body, 2 free)", who, i, p, kind);
      const int lim = kind == 1.0 ? s.nbody : kind == 2.0 ? s.nfree : 1;
      if (!(idx >= 0.0 && idx < (double)lim) || idx != (double)(int)idx)
        return fail(RH_EINVAL, "%s: system %d: point %d: index %g outside [0, %d)", who, i, p, idx, lim);
      nfree += kind == 2.0;
    }
    if (nfree != s.nfree) return fail(RH_EINVAL, "%s: system %d: %d free points in the table, nfree=%d", who, i, nfree, s.nfree);
    for (int l = 0; l < s.nline; ++l) {
      const double pa = s.line_host[RH_MAL_A * s.nline + l], pb = s.line_host[RH_MAL_B * s.nline + l];
      if (!(pa >= 0.0 && pa < (double)s.npoint && pb >= 0.0 && pb < (double)s.npoint) || pa != (double)(int)pa ||
          pb != (double)(int)pb)
        return fail(RH_EINVAL, "%s: system %d: line %d: point index (%g, %g) outside [0, %d)", who, i, l, pa, pb, s.npoint);
      const double tol = s.line_host[RH_MAL_TOL * s.nline + l], dep = s.line_host[RH_MAL_DEPTH * s.nline + l];
      if (!(tol > 0.0) || !(tol < 1.0)) return fail(RH_EINVAL, "%s: system %d: line %d: tol=%g outside (0, 1)", who, i, l, tol);
      if (!(dep == dep)) return fail(RH_EINVAL, "%s: system %d: line %d: depth is NaN", who, i, l);
      if (!(s.line_host[RH_MAL_W * s.nline + l] >= 0.0))
        return fail(RH_EINVAL, "%s: system %d: line %d: W < 0 (buoyant lines are not supported)", who, i, l);
    }
    a.nbm = s.nbody > a.nbm ? s.nbody : a.nbm;
    a.nlm = s.nline > a.nlm ? s.nline : a.nlm;
    a.nfm = s.nfree > a.nfm ? s.nfree : a.nfm;
  }
  a.sys = sys_dev;
  a.nsys = nsys;
  a.n = n;
  a.wsd = rh::moor::arr_ws_doubles(6 * a.nbm, 3 * a.nfm, a.nlm);
  a.gw = 1;
  while (a.gw < a.nlm) a.gw <<= 1;
  while (a.gw < 64 && (size_t)(64 / a.gw) * a.wsd * sizeof(double) > rh::kMoorArrLds) a.gw <<= 1;
  if ((size_t)(64 / a.gw) * a.wsd * sizeof(double) > rh::kMoorArrLds)
    return fail(RH_EINVAL, "%s: a pose's workspace of %d doubles does not fit in LDS", who, a.wsd);
  return RH_OK;
}
}  // namespace

int rh_moor_array_eval(rh_ctx* ctx, const rh_moor_array_system* sys, const rh_moor_array_system* sys_dev, int nsys,
                       int npose, const int* sys_idx, const double* r6, double* warm, double* free_pts, double* F,
                       double* K, double* T, double* J, int* nev, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_moor_array_eval: null context");
  rh::MoorArrLaunch a;
  if (int r = check_moor_array_systems(sys, sys_dev, nsys, npose, "rh_moor_array_eval", a)) return r;
  if (npose == 0) return RH_OK;
  if (!r6 || !warm || !F || !K || !T || !status || (a.nfm > 0 && !free_pts))
    return fail(RH_EINVAL, "rh_moor_array_eval: null r6, warm, free, F, K, T or status");
  a.sys_idx = sys_idx;
  RH_HIP(hipSetDevice(ctx->device));
  const int ppb = 64 / a.gw;
  hipLaunchKernelGGL(rh::k_moor_array_eval, dim3((unsigned)((npose + ppb - 1) / ppb)), dim3(64),
                     (size_t)ppb * a.wsd * sizeof(double), (hipStream_t)stream, a, r6, warm, free_pts, F, K, T, J, nev,
                     status);
  RH_HIP(hipGetLastError());
  return RH_OK;
}

int rh_array_statics_solve(rh_ctx* ctx, const rh_moor_array_system* sys, const rh_moor_array_system* sys_dev, int nsys,
                           int ncase, const int* sys_idx, const double* X_ref, const double* K_hs, const double* F_const,
                           const double* warm0, const double* free0, double* X, double* warm, double* free_pts,
                           int* iters, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_array_statics_solve: null context");
  rh::MoorArrLaunch a;
  if (int r = check_moor_array_systems(sys, sys_dev, nsys, ncase, "rh_array_statics_solve", a)) return r;
  if (ncase == 0) return RH_OK;
  if (!X_ref || !K_hs || !F_const || !X || !warm || !iters || !status || (a.nfm > 0 && (!free0 || !free_pts)))
    return fail(RH_EINVAL, "rh_array_statics_solve: null X_ref, K_hs, F_const, free0, X, warm, free, iters or status");
  a.sys_idx = sys_idx;
  RH_HIP(hipSetDevice(ctx->device));
  const int ppb = 64 / a.gw;
  hipLaunchKernelGGL(rh::k_array_statics_solve, dim3((unsigned)((ncase + ppb - 1) / ppb)), dim3(64),
                     (size_t)ppb * a.wsd * sizeof(double), (hipStream_t)stream, a, X_ref, K_hs, F_const, warm0, free0, X,
                     warm, free_pts, iters, status);
  RH_HIP(hipGetLastError());
  return RH_OK;
}
