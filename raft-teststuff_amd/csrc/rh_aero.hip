// rh_aero.hip -- aero-servo added mass and damping of batched wind cases on the device: the
// kernel over the host/device math of rh_aero.h and its ABI call (rh_rotor_aero_mb).
// Included by rh_abi.hip after its `fail` / RH_HIP helpers.
//
// Mapping: one workgroup of 256 lanes per (case, tile of 128 bins).  The launch is bound by its
// stores (2 x 288 bytes per (case, bin)), so it has two phases around one barrier that sits outside
// every data-dependent branch:
//   1. lanes 0..127 form a(w), b(w) of their bin for every pair of the case in LDS; lanes 128..135
//      form the pairs' bin-independent 6 x 6 patterns P, lane 136 the gyroscopic matrix of the summed
//      vectors, lane 137 (first tile only) the case's mean load f_aero0;
//   2. the lanes sweep the tile's [128][36] outputs flat, two doubles per lane and step, so that a
//      wave writes 1 KiB of contiguous bytes per store (16 bytes per lane; a bin's 36 doubles start
//      at a multiple of 288 bytes = 18 x 16).  Nine steps for M and B each.
// The pairs of a case are found by two searches in the non-decreasing pair_case (25 halvings each,
// every lane the same).  No atomics; every loop has a fixed bound; a bin index past nw is clamped
// where it is read and predicated where it is stored; a row's bits depend on neither the launch
// size nor its neighbours.
#pragma once
#include "rh_common.h"
#include "rh_aero.h"

namespace rh {

constexpr int kAeroTile = 128;      // bins of a workgroup
constexpr int kAeroThreads = 256;
constexpr int kAeroSweep = kAeroTile * 36 / 2 / kAeroThreads;   // steps of two doubles per lane
constexpr int kAeroMaxPairs = RH_AERO_MAX_PAIRS;
static_assert(kAeroSweep * 2 * kAeroThreads == kAeroTile * 36, "the sweep covers the tile exactly");
static_assert(kAeroTile + kAeroMaxPairs + 2 <= kAeroThreads, "phase 1 has a lane for every job");
static_assert(aero::kMode == RH_AP_MODE && aero::kRq == RH_AP_RQ && aero::kRhub == RH_AP_RHUB &&
                  aero::kIdrive == RH_AP_I_DRIVETRAIN && aero::kNg == RH_AP_NG && aero::kKfloat == RH_AP_K_FLOAT &&
                  aero::kKpBeta == RH_AP_KP_BETA && aero::kKiBeta == RH_AP_KI_BETA && aero::kKpTau == RH_AP_KP_TAU &&
                  aero::kKiTau == RH_AP_KI_TAU && aero::kGyro == RH_AP_GYRO && aero::kParamCount == RH_AP_COUNT,
              "rh_aero.h and rafthip.h agree on the parameter row");

// grid ncase * ntile (tile fastest), block kAeroThreads
__global__ __launch_bounds__(kAeroThreads) void k_rotor_aero_mb(int ncase, int npair, int nw, int ntile,
                                                                const double* __restrict__ w,
                                                                const int* __restrict__ pair_case,
                                                                const double* __restrict__ loads,
                                                                const double* __restrict__ dloads,
                                                                const double* __restrict__ param,
                                                                const double* __restrict__ M0,
                                                                const double* __restrict__ B0, int base_per_bin,
                                                                double* __restrict__ M, double* __restrict__ B,
                                                                double* __restrict__ f_aero0) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sP[kAeroMaxPairs][36];
  __shared__ __attribute__((aligned(16))) double sG[36];
  __shared__ double sA[kAeroMaxPairs][kAeroTile];
  __shared__ double sB[kAeroMaxPairs][kAeroTile];
  const int t = threadIdx.x;
  const int cb = (int)(blockIdx.x / (unsigned)ntile);
  const int tile = (int)(blockIdx.x - (unsigned)cb * (unsigned)ntile);
  const bool live = cb < ncase;                    // the grid is ncase * ntile blocks
  const int c = live ? cb : ncase - 1;
  const int bin0 = tile * kAeroTile;
  const int first = aero::first_at_least(pair_case, npair, c);
  const int past = aero::first_at_least(pair_case, npair, c + 1);
  const int np = past - first < kAeroMaxPairs ? past - first : kAeroMaxPairs;   // (the host refused more)

  if (t < kAeroTile) {
    const int bin = bin0 + t < nw ? bin0 + t : nw - 1;
    const double wb = w[bin];
#pragma unroll 1
    for (int k = 0; k < kAeroMaxPairs; ++k) {
      if (k < np) {
        const double* par = param + (size_t)(first + k) * RH_AP_COUNT;
        const aero::Derivs d = aero::load_derivs(dloads + (size_t)(first + k) * 6);
        double a, b;
        aero::bin_coefficients(par, d, wb, a, b);
        sA[k][t] = a;
        sB[k][t] = b;
      }
    }
  } else if (t < kAeroTile + kAeroMaxPairs) {
    const int k = t - kAeroTile;
    if (k < np) {
      double P[36];
      aero::pattern(param + (size_t)(first + k) * RH_AP_COUNT, P);
#pragma unroll
      for (int e = 0; e < 36; ++e) sP[k][e] = P[e];
    }
  } else if (t == kAeroTile + kAeroMaxPairs) {
    double g[3] = {0.0, 0.0, 0.0}, G[36];
#pragma unroll 1
    for (int k = 0; k < kAeroMaxPairs; ++k) {
      if (k < np) {
        const double* par = param + (size_t)(first + k) * RH_AP_COUNT;
        g[0] += par[RH_AP_GYRO + 0], g[1] += par[RH_AP_GYRO + 1], g[2] += par[RH_AP_GYRO + 2];
      }
    }
    aero::gyro_matrix(g, G);
#pragma unroll
    for (int e = 0; e < 36; ++e) sG[e] = G[e];
  } else if (t == kAeroTile + kAeroMaxPairs + 1) {
    if (tile == 0) {
      double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int k = 0; k < kAeroMaxPairs; ++k) {
        if (k < np) {
          double f6[6];
          aero::mean_load(param + (size_t)(first + k) * RH_AP_COUNT, loads + (size_t)(first + k) * 8, f6);
#pragma unroll
          for (int e = 0; e < 6; ++e) f[e] += f6[e];
        }
      }
      if (live) {
#pragma unroll
        for (int e = 0; e < 6; ++e) f_aero0[(size_t)c * 6 + e] = f[e];
      }
    }
  }
  __syncthreads();

  double* __restrict__ Mc = M + ((size_t)c * nw + bin0) * 36;
  double* __restrict__ Bc = B + ((size_t)c * nw + bin0) * 36;
#pragma unroll
  for (int it = 0; it < kAeroSweep; ++it) {
    const int e = 2 * (it * kAeroThreads + t);   // < kAeroTile * 36, even: e and e + 1 are entries of one bin
    const int bl = e / 36, ij = e - bl * 36;
    if (live && bin0 + bl < nw) {
      const size_t src = (base_per_bin ? (size_t)(bin0 + bl) * 36 : (size_t)0) + ij;
      const double m0x = M0[src], m0y = M0[src + 1], b0x = B0[src], b0y = B0[src + 1];
      double2 m, b;
      m.x = aero::entry(np, kAeroMaxPairs, &sA[0][bl], kAeroTile, &sP[0][ij], m0x);
      m.y = aero::entry(np, kAeroMaxPairs, &sA[0][bl], kAeroTile, &sP[0][ij + 1], m0y);
      b.x = aero::damping_entry(np, kAeroMaxPairs, &sB[0][bl], kAeroTile, &sP[0][ij], b0x, sG[ij]);
      b.y = aero::damping_entry(np, kAeroMaxPairs, &sB[0][bl], kAeroTile, &sP[0][ij + 1], b0y, sG[ij + 1]);
      *reinterpret_cast<double2*>(Mc + e) = m;
      *reinterpret_cast<double2*>(Bc + e) = b;
    }
  }
}

}  // namespace rh

int rh_rotor_aero_mb(rh_ctx* ctx, int ncase, int npair, int nw, const double* w, const int* pair_case,
                     const int* pair_case_host, const int* pair_mode_host, const double* loads, const double* dloads,
                     const double* param, const double* M0, const double* B0, int base_per_bin, double* M, double* B,
                     double* f_aero0, rh_stream stream) {
  const char* who = "rh_rotor_aero_mb";
  if (!ctx) return fail(RH_EINVAL, "%s: null context", who);
  if (ncase < 1 || npair < 1 || nw < 1)
    return fail(RH_EINVAL, "%s: ncase=%d, npair=%d and nw=%d must be >= 1", who, ncase, npair, nw);
  if (npair > (1 << 24) || ncase > (1 << 24)) return fail(RH_EINVAL, "%s: more than 2^24 pairs or cases", who);
  if (!w || !pair_case || !pair_case_host || !pair_mode_host || !loads || !dloads || !param)
    return fail(RH_EINVAL, "%s: null w, pair_case, pair_case_host, pair_mode_host, loads, dloads or param", who);
  if (!M0 || !B0 || !M || !B || !f_aero0) return fail(RH_EINVAL, "%s: null M0, B0, M, B or f_aero0", who);
  if (((uintptr_t)M | (uintptr_t)B) & 15) return fail(RH_EINVAL, "%s: M and B must be 16-byte aligned", who);
  int run = 0;
  for (int p = 0; p < npair; ++p) {
    const int c = pair_case_host[p];
    if (c < 0 || c >= ncase) return fail(RH_EINVAL, "%s: pair %d: case row %d outside [0, %d)", who, p, c, ncase);
    if (p > 0 && c < pair_case_host[p - 1])
      return fail(RH_EINVAL, "%s: pair %d: pair_case decreases (%d after %d)", who, p, c, pair_case_host[p - 1]);
    run = (p > 0 && c == pair_case_host[p - 1]) ? run + 1 : 1;
    if (run > RH_AERO_MAX_PAIRS)
      return fail(RH_EINVAL, "%s: case row %d has more than %d pairs", who, c, RH_AERO_MAX_PAIRS);
    if (pair_mode_host[p] != 1 && pair_mode_host[p] != 2)
      return fail(RH_EINVAL, "%s: pair %d: aeroServoMod %d (1 or 2)", who, p, pair_mode_host[p]);
  }
  const int ntile = (nw + rh::kAeroTile - 1) / rh::kAeroTile;
  if ((long long)ncase * ntile > 0x7fffffffLL) return fail(RH_EINVAL, "%s: ncase x bin tiles exceeds 2^31 - 1", who);
  RH_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(rh::k_rotor_aero_mb, dim3((unsigned)(ncase * ntile)), dim3(rh::kAeroThreads), 0, (hipStream_t)stream,
                     ncase, npair, nw, ntile, w, pair_case, loads, dloads, param, M0, B0, base_per_bin, M, B, f_aero0);
  RH_HIP(hipGetLastError());
  return RH_OK;
}
