// rh_channels.hip -- turbine output channels of batched cases on the device: the kernel over the
// host/device math of rh_channels.h and its ABI call (rh_turbine_channels).
// Included by rh_abi.hip after rh_aero.hip.
//
// Mapping: one workgroup of 256 lanes per case; the lanes stride the bins.  The launch is bound by
// its Xi loads (surge and pitch of every row and bin, 32 bytes) and its PSD stores (5 x 8 bytes per
// rotor and bin), both coalesced along the bins.  For each rotor of the case (a uniform loop), every
// lane forms the bin's coefficients once (a(w), b(w), C(w) of the rotor's pair, if it has one) and
// then walks the response rows; the five sums of |x|^2 of a rotor stay in registers, go through a wave
// reduction and are left in LDS per wave.  One barrier after the rotor loop, outside every
// data-dependent branch; then lane k sums the four waves' parts of (rotor, channel) k in a fixed
// order.  With one rotor (every design the project ships) surge and pitch are read once; a further
// rotor reads them again, from cache.  The pairs of a case are found by two searches in the
// non-decreasing pair_case and the rotor's pair among them by a loop of RH_AERO_MAX_PAIRS steps
// (every lane the same).  No atomics; every loop has a fixed or uniform bound; a bin index past nw is
// clamped where it is read and predicated where it is stored or summed; a case's bits depend on
// neither the launch size nor its neighbours.
#pragma once
#include "rh_common.h"
#include "rh_channels.h"

namespace rh {

constexpr int kChanThreads = 256;
constexpr int kChanWaves = kChanThreads / 64;
constexpr int kChanMaxRotors = RH_CHAN_MAX_ROTORS;
static_assert(chan::kZhub == RH_CP_ZHUB && chan::kKpTau == RH_CP_KP_TAU && chan::kKiTau == RH_CP_KI_TAU &&
                  chan::kPairCount == RH_CP_COUNT && chan::kZrel == RH_CG_ZREL && chan::kMt == RH_CG_MT &&
                  chan::kZcg == RH_CG_ZCG && chan::kHarm == RH_CG_HARM && chan::kIcg == RH_CG_ICG &&
                  chan::kG == RH_CG_G && chan::kZbase == RH_CG_ZBASE && chan::kHasTower == RH_CG_HAS_TOWER &&
                  chan::kGeomCount == RH_CG_COUNT && chan::kAxRNA == RH_TC_AXRNA && chan::kMbase == RH_TC_MBASE &&
                  chan::kOmega == RH_TC_OMEGA && chan::kTorque == RH_TC_TORQUE && chan::kBPitch == RH_TC_BPITCH &&
                  chan::kPower == RH_TC_POWER && chan::kSpectra == RH_TC_SPECTRA && chan::kMeans == RH_TC_COUNT,
              "rh_channels.h and rafthip.h agree on the rows and the channel order");
static_assert(kChanMaxRotors * chan::kSpectra <= kChanThreads, "a lane for every (rotor, channel) sum");

// grid ncase, block kChanThreads
__global__ __launch_bounds__(kChanThreads) void k_turbine_channels(
    int nrow, int nw, double dw, const double* __restrict__ w, const rh_c128* __restrict__ Xi,
    const double* __restrict__ pitch0, int nrot, const double* __restrict__ geom, int npair,
    const int* __restrict__ pair_case, const int* __restrict__ pair_rotor, const double* __restrict__ loads,
    const double* __restrict__ dloads, const double* __restrict__ param, const double* __restrict__ op,
    const double* __restrict__ pair_row, const int* __restrict__ pair_vw, const double* __restrict__ V_w,
    double* __restrict__ psd, double* __restrict__ stdv, double* __restrict__ avg) {
#pragma clang fp contract(off)
  __shared__ double sred[kChanWaves][kChanMaxRotors * chan::kSpectra];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int c = blockIdx.x;
  int first = 0, past = 0;
  if (npair > 0) {
    first = aero::first_at_least(pair_case, npair, c);
    past = aero::first_at_least(pair_case, npair, c + 1);
  }
  const double sp0 = pitch0 ? sin(pitch0[c]) : 0.0;
  const int nstep = (nw + kChanThreads - 1) / kChanThreads;
  const rh_c128* __restrict__ Xc = Xi + (size_t)c * nrow * 6 * nw;

#pragma unroll 1
  for (int ir = 0; ir < nrot; ++ir) {
    const int p = chan::pair_of_rotor(pair_rotor, first, past, RH_AERO_MAX_PAIRS, ir);
    const chan::Rotor r = chan::rotor_of(geom + (size_t)ir * RH_CG_COUNT, p >= 0 ? param + (size_t)p * RH_AP_COUNT : nullptr,
                                         p >= 0 ? dloads + (size_t)p * 6 : nullptr,
                                         p >= 0 ? pair_row + (size_t)p * RH_CP_COUNT : nullptr);
    const double* __restrict__ vrow = r.mode == 2 ? V_w + (size_t)pair_vw[p] * nw : nullptr;
    if (t == 0) {
      double a6[chan::kMeans];
      chan::means(r, sp0, p >= 0 ? loads + (size_t)p * 8 : nullptr, p >= 0 ? op + (size_t)p * 5 : nullptr, a6);
#pragma unroll
      for (int k = 0; k < chan::kMeans; ++k) avg[((size_t)c * nrot + ir) * chan::kMeans + k] = a6[k];
    }
    double ss[chan::kSpectra] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int it = 0; it < nstep; ++it) {
      const int b = it * kChanThreads + t;
      const bool live = b < nw;
      const int bc = live ? b : nw - 1;
      const chan::Bin bin = chan::bin_of(r, w[bc]);
      double pp[chan::kSpectra] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int row = 0; row < nrow; ++row) {
        const rh_c128* X = Xc + (size_t)row * 6 * nw + bc;
        const cd xs = ld(X), xp = ld(X + (size_t)4 * nw);
        double m2[chan::kSpectra];
        chan::row_abs2(r, bin, xs.r, xs.i, xp.r, xp.i, m2);
#pragma unroll
        for (int k = 0; k < chan::kSpectra; ++k) {
          pp[k] += chan::psd_term(m2[k], dw);
          ss[k] += live ? m2[k] : 0.0;
        }
      }
      if (vrow) {     // (uniform) the wind row of a closed control loop
        double m2[chan::kSpectra];
        chan::wind_abs2(r, bin, vrow[bc], m2);
#pragma unroll
        for (int k = chan::kOmega; k < chan::kSpectra; ++k) {
          pp[k] += chan::psd_term(m2[k], dw);
          ss[k] += live ? m2[k] : 0.0;
        }
      }
      if (psd && live) {
#pragma unroll
        for (int k = 0; k < chan::kSpectra; ++k)
          psd[(((size_t)c * nrot + ir) * chan::kSpectra + k) * nw + b] = chan::psd_units(k, pp[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < chan::kSpectra; ++k) {
      const double s = wave_sum(ss[k]);
      if (lane == 0) sred[wv][ir * chan::kSpectra + k] = s;
    }
  }
  __syncthreads();
  if (t < nrot * chan::kSpectra) {
    double s = sred[0][t];
#pragma unroll
    for (int i = 1; i < kChanWaves; ++i) s += sred[i][t];
    stdv[(size_t)c * nrot * chan::kSpectra + t] = chan::rms_units(t % chan::kSpectra, sqrt(0.5 * s));
  }
}

}  // namespace rh

int rh_turbine_channels(rh_ctx* ctx, int ncase, int nrow, int nw, double dw, const double* w, const rh_c128* Xi,
                        const double* pitch0, int nrot, const double* geom, int npair, const int* pair_case,
                        const int* pair_case_host, const int* pair_rotor, const int* pair_rotor_host,
                        const int* pair_mode_host, const double* loads, const double* dloads, const double* param,
                        const double* op, const double* pair_row, const int* pair_vw, const int* pair_vw_host, int nvw,
                        const double* V_w, double* psd, double* stdv, double* avg, rh_stream stream) {
  const char* who = "rh_turbine_channels";
  namespace C = rh::chan;
  if (!ctx) return fail(RH_EINVAL, "%s: null context", who);
  if (ncase < 1 || nrow < 1 || nw < 1 || nrot < 1)
    return fail(RH_EINVAL, "%s: ncase=%d, nrow=%d, nw=%d and nrot=%d must be >= 1", who, ncase, nrow, nw, nrot);
  if (npair < 0 || (npair > 0 && nvw < 1))
    return fail(RH_EINVAL, "%s: npair=%d must be >= 0 and, with pairs, nvw=%d >= 1", who, npair, nvw);
  if (nrot > RH_CHAN_MAX_ROTORS) return fail(RH_EINVAL, "%s: nrot=%d (at most %d)", who, nrot, RH_CHAN_MAX_ROTORS);
  if (npair > (1 << 24) || ncase > (1 << 24)) return fail(RH_EINVAL, "%s: more than 2^24 pairs or cases", who);
  if (!(dw > 0.0)) return fail(RH_EINVAL, "%s: dw=%g must be > 0", who, dw);
  if (!w || !Xi || !geom || !stdv || !avg) return fail(RH_EINVAL, "%s: null w, Xi, geom, std or avg", who);
  if (npair > 0) {
    if (!pair_case || !pair_case_host || !pair_rotor || !pair_rotor_host || !pair_mode_host || !pair_vw || !pair_vw_host)
      return fail(RH_EINVAL, "%s: null pair_case, pair_rotor, pair_mode_host or pair_vw column (device or host copy)", who);
    if (!loads || !dloads || !param || !op || !pair_row || !V_w)
      return fail(RH_EINVAL, "%s: null loads, dloads, param, op, pair_row or V_w", who);
    int p = 0;
    switch (C::check_pairs(ncase, nrot, npair, nvw, RH_AERO_MAX_PAIRS, pair_case_host, pair_rotor_host, pair_mode_host,
                           pair_vw_host, &p)) {
      case C::kFine: break;
      case C::kCaseRange:
        return fail(RH_EINVAL, "%s: pair %d: case row %d outside [0, %d)", who, p, pair_case_host[p], ncase);
      case C::kCaseDecreases:
        return fail(RH_EINVAL, "%s: pair %d: pair_case decreases (%d after %d)", who, p, pair_case_host[p],
                    pair_case_host[p - 1]);
      case C::kTooManyPairs:
        return fail(RH_EINVAL, "%s: case row %d has more than %d pairs", who, pair_case_host[p], RH_AERO_MAX_PAIRS);
      case C::kMode: return fail(RH_EINVAL, "%s: pair %d: aeroServoMod %d (1 or 2)", who, p, pair_mode_host[p]);
      case C::kRotorRange:
        return fail(RH_EINVAL, "%s: pair %d: rotor %d outside [0, %d)", who, p, pair_rotor_host[p], nrot);
      case C::kRotorTwice:
        return fail(RH_EINVAL, "%s: pair %d: case row %d names rotor %d twice", who, p, pair_case_host[p],
                    pair_rotor_host[p]);
      default: return fail(RH_EINVAL, "%s: pair %d: V_w row %d outside [0, %d)", who, p, pair_vw_host[p], nvw);
    }
  }
  RH_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(rh::k_turbine_channels, dim3((unsigned)ncase), dim3(rh::kChanThreads), 0, (hipStream_t)stream, nrow,
                     nw, dw, w, Xi, pitch0, nrot, geom, npair, pair_case, pair_rotor, loads, dloads, param, op, pair_row,
                     pair_vw, V_w, psd, stdv, avg);
  RH_HIP(hipGetLastError());
  return RH_OK;
}
