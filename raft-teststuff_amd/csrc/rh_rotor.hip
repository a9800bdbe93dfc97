// rh_rotor.hip -- rotor blade-element momentum loads on the device: the kernel over the
// host/device math of rh_rotor.h and its ABI call (rh_rotor_loads).
// Included by rh_abi.hip after its `fail` / RH_HIP helpers.
//
// Mapping: one workgroup per operating point, one lane per (sector, section).  The sections of a
// sector sit in adjacent lanes of a group of gw = the next power of two >= the call's largest nr
// (gw <= 64, so a group never straddles a wave); the groups of the sectors fill the workgroup
// (ns_max gw <= 1024 lanes, rounded up to whole waves).  Lanes past a rotor's nr or nsector are
// padding: they read clamped addresses and contribute zeros.  The inflow, the Brent solve, the
// loads and the derivative evaluations are a lane's own (rh_rotor.h); the Brent loop runs to the
// wave's vote, finished lanes predicated off.  The 11 sums along the blade go across the group with
// __shfl_xor butterflies, each sector's sums to LDS, and after the workgroup's one barrier (outside
// every data-dependent branch) lane 0 combines the sectors in sector order.  No atomics; a point's
// bits depend on neither the launch size nor its neighbours.  The spline and section tables are
// tens of KB per rotor and are read through the cache.
#pragma once
#include "rh_common.h"
#include "rh_rotor.h"

namespace rh {

constexpr int kRotorPart = rotor::kSums + 1;   // the sums of a sector and its status

// grid npoint, block = ns_max gw rounded up to whole waves (<= MAXT)
template <int MAXT>
__global__ __launch_bounds__(MAXT) void k_rotor_loads(const rh_rotor* __restrict__ rot, int nrot, int npoint, int gw,
                                                      int nr_max, int ns_max, const int* __restrict__ rot_idx,
                                                      const double* __restrict__ op, double* __restrict__ loads,
                                                      double* __restrict__ dloads, double* __restrict__ sec,
                                                      int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double part[RH_ROTOR_MAX_SECTORS][kRotorPart];
  const int p = blockIdx.x < (unsigned)npoint ? (int)blockIdx.x : npoint - 1;   // the grid is npoint blocks
  const int t = threadIdx.x;
  const int j = t / gw;        // sector
  const int i = t - j * gw;    // section
  const int ri = rot_idx ? rot_idx[p] : 0;
  const bool rot_ok = ri >= 0 && ri < nrot;
  const rh_rotor R = rot[rot_ok ? ri : 0];
  const int nr = R.nr, ns = R.nsector;
  const bool run = rot_ok && j < ns && i < nr;
  double weight, cone_path;
  const rotor::Section S = rotor::load_section(R.section, R.nknot, R.knots, R.coef, nr, R.kx, R.knot_stride, i, weight,
                                               cone_path);
  rotor::Blade B;
  B.Rhub = R.Rhub, B.Rtip = R.Rtip, B.rho = R.rho, B.mu = R.mu, B.hubHt = R.hubHt, B.shearExp = R.shearExp;
  B.B = R.B;
  B.usecd = R.usecd != 0, B.tiploss = R.tiploss != 0, B.hubloss = R.hubloss != 0, B.wakerotation = R.wakerotation != 0;
  const double Uinf = op[(size_t)p * 5 + 0], Omega = op[(size_t)p * 5 + 1], pitch_deg = op[(size_t)p * 5 + 2];
  const double tilt = op[(size_t)p * 5 + 3], yaw = op[(size_t)p * 5 + 4];
  const int jj = j < ns ? j : ns - 1;
  const double azimuth = (360.0 * (double)jj / ns) * rotor::kDeg2Rad;

  rotor::PointOut o;
  rotor::section_point(B, S, Uinf, Omega, pitch_deg, tilt, yaw, azimuth, dloads != nullptr, run, o);

  double v[rotor::kSums];
  rotor::section_terms(o, weight, S.z_az, cone_path, azimuth, v);
  int st = run ? o.status : 0;
#pragma unroll
  for (int k = 0; k < rotor::kSums; ++k) {
    double x = run ? v[k] : 0.0;
    for (int m = 1; m < gw; m <<= 1) x += __shfl_xor(x, m);
    v[k] = x;
  }
  for (int m = 1; m < gw; m <<= 1) {
    const int other = __shfl_xor(st, m);
    st = other > st ? other : st;
  }
  if (i == 0 && j < ns_max && j < RH_ROTOR_MAX_SECTORS) {
#pragma unroll
    for (int k = 0; k < rotor::kSums; ++k) part[j][k] = v[k];
    part[j][rotor::kSums] = (double)st;
  }
  if (sec && j < ns_max && i < nr_max) {
    double* q = sec + (((size_t)p * ns_max + j) * nr_max + i) * 3;
    q[0] = run ? o.phi : 0.0;
    q[1] = run ? o.Np : 0.0;
    q[2] = run ? o.Tp : 0.0;
  }
  __syncthreads();
  if (t == 0) {
    double L[8], D[6];
    int s = rotor::kOk;
    if (rot_ok) {
      const int nsc = ns < ns_max ? ns : ns_max;
      s = rotor::combine_sectors(&part[0][0], kRotorPart, nsc, R.B, Omega, L, dloads ? D : nullptr);
      for (int k = 0; k < nsc; ++k) {
        const int sk = (int)part[k][rotor::kSums];
        s = sk > s ? sk : s;
      }
    } else {
      s = rotor::kBadRotor;
#pragma unroll
      for (int k = 0; k < 8; ++k) L[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) D[k] = 0.0;
    }
    if (blockIdx.x < (unsigned)npoint) {
#pragma unroll
      for (int k = 0; k < 8; ++k) loads[(size_t)p * 8 + k] = L[k];
      if (dloads) {
#pragma unroll
        for (int k = 0; k < 6; ++k) dloads[(size_t)p * 6 + k] = D[k];
      }
      status[p] = s;
    }
  }
}

}  // namespace rh

namespace {
// validates the host records; returns the group width and the largest nr and nsector
int check_rotors(const rh_rotor* rot, const rh_rotor* rot_dev, int nrot, int npoint, int& gw, int& nr_max, int& ns_max) {
  const char* who = "rh_rotor_loads";
  if (!rot || !rot_dev) return fail(RH_EINVAL, "%s: null rotor array", who);
  if (nrot < 1) return fail(RH_EINVAL, "%s: nrot=%d must be >= 1", who, nrot);
  if (npoint < 0 || npoint > (1 << 24)) return fail(RH_EINVAL, "%s: %d points outside [0, 2^24]", who, npoint);
  nr_max = ns_max = 0;
  for (int n = 0; n < nrot; ++n) {
    const rh_rotor& r = rot[n];
    if (r.nr < 1 || r.nr > RH_ROTOR_MAX_SECTIONS)
      return fail(RH_EINVAL, "%s: rotor %d: nr=%d outside [1, %d]", who, n, r.nr, RH_ROTOR_MAX_SECTIONS);
    if (r.nsector < 1 || r.nsector > RH_ROTOR_MAX_SECTORS)
      return fail(RH_EINVAL, "%s: rotor %d: nsector=%d outside [1, %d]", who, n, r.nsector, RH_ROTOR_MAX_SECTORS);
    if (r.B < 1) return fail(RH_EINVAL, "%s: rotor %d: B=%d must be >= 1", who, n, r.B);
    if (r.kx < 1 || r.kx > rh::rotor::kMaxDegree)
      return fail(RH_EINVAL, "%s: rotor %d: spline degree kx=%d outside [1, %d]", who, n, r.kx, rh::rotor::kMaxDegree);
    const int kmin = 2 * (r.kx + 1);
    if (r.knot_stride < kmin || r.knot_stride > RH_ROTOR_MAX_KNOTS)
      return fail(RH_EINVAL, "%s: rotor %d: knot_stride=%d outside [%d, %d]", who, n, r.knot_stride, kmin,
                  RH_ROTOR_MAX_KNOTS);
    if (!r.section || !r.nknot || !r.knots || !r.coef || !r.section_host || !r.nknot_host || !r.knots_host ||
        !r.coef_host)
      return fail(RH_EINVAL, "%s: rotor %d: null table", who, n);
    if (!(r.Rhub > 0.0) || !(r.Rtip > r.Rhub) || !(r.mu > 0.0) || !(r.rho > 0.0) || !(r.hubHt == r.hubHt) ||
        r.hubHt == 0.0 || !(r.shearExp == r.shearExp))
      return fail(RH_EINVAL, "%s: rotor %d: Rhub, Rtip, rho, mu, hubHt or shearExp out of range", who, n);
    for (int i = 0; i < r.nr; ++i)
      if (!(r.section_host[RH_RS_R * r.nr + i] > 0.0))
        return fail(RH_EINVAL, "%s: rotor %d: station %d: r must be > 0", who, n, i);
    for (int row = 0; row < 2 * r.nr; ++row) {
      const int nx = r.nknot_host[row];
      if (nx < kmin || nx > r.knot_stride)
        return fail(RH_EINVAL, "%s: rotor %d: spline %d: %d knots outside [%d, %d]", who, n, row, nx, kmin, r.knot_stride);
      const double* tx = r.knots_host + (size_t)row * (r.knot_stride + 4);
      const double* ty = tx + r.knot_stride;
      for (int k = 1; k < nx; ++k)
        if (!(tx[k] >= tx[k - 1])) return fail(RH_EINVAL, "%s: rotor %d: spline %d: alpha knots decrease", who, n, row);
      if (!(tx[nx - r.kx - 1] > tx[r.kx]))
        return fail(RH_EINVAL, "%s: rotor %d: spline %d: empty alpha knot range", who, n, row);
      if (!(ty[1] >= ty[0]) || !(ty[2] > ty[1]) || !(ty[3] >= ty[2]))
        return fail(RH_EINVAL, "%s: rotor %d: spline %d: Re knots do not increase", who, n, row);
    }
    nr_max = r.nr > nr_max ? r.nr : nr_max;
    ns_max = r.nsector > ns_max ? r.nsector : ns_max;
  }
  gw = 1;
  while (gw < nr_max) gw <<= 1;
  return RH_OK;
}
}  // namespace

int rh_rotor_loads(rh_ctx* ctx, const rh_rotor* rot, const rh_rotor* rot_dev, int nrot, int npoint, const int* rot_idx,
                   const double* op, double* loads, double* dloads, double* sec, int* status, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_rotor_loads: null context");
  int gw, nr_max, ns_max;
  if (int r = check_rotors(rot, rot_dev, nrot, npoint, gw, nr_max, ns_max)) return r;
  if (!op || !loads || !status) return fail(RH_EINVAL, "rh_rotor_loads: null op, loads or status");
  if (npoint == 0) return RH_OK;
  RH_HIP(hipSetDevice(ctx->device));
  const int threads = ((ns_max * gw + 63) / 64) * 64;   // <= 16 x 64
  if (threads <= 256)
    hipLaunchKernelGGL(rh::k_rotor_loads<256>, dim3((unsigned)npoint), dim3(threads), 0, (hipStream_t)stream, rot_dev, nrot,
                       npoint, gw, nr_max, ns_max, rot_idx, op, loads, dloads, sec, status);
  else
    hipLaunchKernelGGL(rh::k_rotor_loads<1024>, dim3((unsigned)npoint), dim3(threads), 0, (hipStream_t)stream, rot_dev,
                       nrot, npoint, gw, nr_max, ns_max, rot_idx, op, loads, dloads, sec, status);
  RH_HIP(hipGetLastError());
  return RH_OK;
}
