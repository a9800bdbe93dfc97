// rh_bem.hip -- the device side of the potential-flow (BEM) wave excitation of designs that
// bring first-order coefficient files (potFirstOrder = 1; raft/raft_fowt.py:1039-1093).
//
// Per (output heading, bin): bracket the wave heading in the file's headings, blend the two
// excitation coefficient vectors (each stored in its own heading's wave frame), rotate back to
// the global frame by the wave heading and apply the phase of the FOWT's position in the array.
// The result is per unit wave amplitude, like the strip-theory table `finer` it is added to:
//   fbem [nh][6][nw]   F_BEM / zeta of FOWT.calcHydroExcitation
//   fexc [nh][6][nw]   finer + fbem: the `finer` a BEM design's descriptor points at, so every
//                      solver path takes its unit-amplitude excitation from one table
// FP64 VALU, a few dozen operations and 13 complex loads / 12 stores per lane; bins run along
// the lane index, so every load and store of a wave is one contiguous 1 KiB row segment.
#pragma once
#include "rh_common.h"

namespace rh {

// The reference's bracket search (raft/raft_fowt.py:1054-1072), comparisons included: `<=` the
// first heading and `>=` the last one wrap around 360 deg, else the first heading above beta.
// Returns f2; f1 = 1 - f2 is formed by the caller as the reference forms it.
__device__ __forceinline__ double bem_bracket(const double* __restrict__ hd, int nhb, double beta, int& i1, int& i2) {
  const double h0 = hd[0], hl = hd[nhb - 1];
  i1 = nhb - 1;
  i2 = 0;
  if (beta <= h0) {
    const double hlast = hl - 360.0;
    return (beta - hlast) / (h0 - hlast);
  }
  if (beta >= hl) {
    const double hfirst = h0 + 360.0;
    return (beta - hl) / (hfirst - hl);
  }
  for (int i = 0; i < nhb - 1; ++i) {
    if (hd[i + 1] > beta) {
      i1 = i;
      i2 = i + 1;
      return (beta - hd[i]) / (hd[i + 1] - hd[i]);
    }
  }
  return 0.0;   // not reached: hd[nhb-1] > beta holds here
}

// Python's float `%` with a positive divisor (np.remainder): the result takes the divisor's sign.
__device__ __forceinline__ double pymod360(double a) {
  double r = fmod(a, 360.0);
  if (r != 0.0) {
    if (r < 0.0) r += 360.0;
  } else {
    r = 0.0;
  }
  return r;
}

__device__ __forceinline__ void bem_excitation_lane(const rh_bem_design& d, int ih, int b) {
#pragma clang fp contract(off)   // the reference's roundings: no fused multiply-add
  const int nw = d.nw;
  const double beta = d.beta[ih];                                       // wave heading [rad]
  const double bdeg = pymod360(beta * kRad2Deg - d.heading_adjust_deg);  // (np.degrees(beta) - heading_adjust) % 360
  int i1, i2;
  const double f2 = bem_bracket(d.headings_deg, d.nhb, bdeg, i1, i2);
  const double f1 = 1.0 - f2;
  double sb, cb;
  sincos(beta, &sb, &cb);
  // phase of the FOWT's position: exp(-1j k (x_ref cos(beta) + y_ref sin(beta)))
  const double arg = (-d.k[b]) * (d.x_ref * cb + d.y_ref * sb);
  double sp, cp;
  sincos(arg, &sp, &cp);
  const cd ph = mk(cp, sp);
  const rh_c128* X1 = d.X + ((size_t)i1 * 6) * nw + b;
  const rh_c128* X2 = d.X + ((size_t)i2 * 6) * nw + b;
  cd xp[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) xp[c] = add(scl(ld(X1 + (size_t)c * nw), f1), scl(ld(X2 + (size_t)c * nw), f2));
  cd xg[6];
  xg[0] = sub(scl(xp[0], cb), scl(xp[1], sb));
  xg[1] = add(scl(xp[0], sb), scl(xp[1], cb));
  xg[2] = xp[2];
  xg[3] = sub(scl(xp[3], cb), scl(xp[4], sb));
  xg[4] = add(scl(xp[3], sb), scl(xp[4], cb));
  xg[5] = xp[5];
  const size_t o = ((size_t)ih * 6) * nw + b;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const cd f = mul(xg[c], ph);
    const size_t e = o + (size_t)c * nw;
    st(d.fbem + e, f);
    st(d.fexc + e, add(ld(d.finer + e), f));
  }
}

// grid (ceil(nw / 256), nh), 256 threads: one lane per (heading, bin)
__global__ __launch_bounds__(256) void k_bem_excitation(rh_bem_design d) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int ih = blockIdx.y;
  if (b >= d.nw || ih >= d.nh) return;
  bem_excitation_lane(d, ih, b);
}

// grid (ceil(max nw / 256), max nh, ndesign): the same lanes for many designs; nhb = 0 skips one
__global__ __launch_bounds__(256) void k_bem_excitation_batch(const rh_bem_design* __restrict__ designs) {
  const rh_bem_design d = designs[blockIdx.z];
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int ih = blockIdx.y;
  if (d.nhb <= 0 || b >= d.nw || ih >= d.nh) return;
  bem_excitation_lane(d, ih, b);
}

}  // namespace rh
