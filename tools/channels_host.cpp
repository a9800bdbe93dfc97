// Host build of rh_channels.h for the CPU check against raft/fowt.py and raft/rotor.py
// (tests/test_channels_host.py): the same control transfer function, channel arithmetic, means and
// pair-column checks the device runs, walked case after case, rotor after rotor and bin after bin
// instead of by workgroups.
// With -DCHANNELS_HOST_MAIN it is a stand-alone program that runs built-in tables through both
// modes, a case without a pair, two rotors on a case, nw = 1 and 67, nrow = 1 and 3, a batch without
// pairs and refused tables (for a sanitizer run on the CPU):
// g++ -O1 -g -fsanitize=address,undefined -DCHANNELS_HOST_MAIN.
#include "../raft-teststuff_amd/csrc/rh_channels.h"
#include "../include/rafthip.h"

namespace A = rh::aero;
namespace C = rh::chan;
static_assert(C::kZhub == RH_CP_ZHUB && C::kKpTau == RH_CP_KP_TAU && C::kKiTau == RH_CP_KI_TAU &&
                  C::kPairCount == RH_CP_COUNT && C::kZrel == RH_CG_ZREL && C::kMt == RH_CG_MT && C::kZcg == RH_CG_ZCG &&
                  C::kHarm == RH_CG_HARM && C::kIcg == RH_CG_ICG && C::kG == RH_CG_G && C::kZbase == RH_CG_ZBASE &&
                  C::kHasTower == RH_CG_HAS_TOWER && C::kGeomCount == RH_CG_COUNT && C::kAxRNA == RH_TC_AXRNA &&
                  C::kMbase == RH_TC_MBASE && C::kOmega == RH_TC_OMEGA && C::kTorque == RH_TC_TORQUE &&
                  C::kBPitch == RH_TC_BPITCH && C::kPower == RH_TC_POWER && C::kSpectra == RH_TC_SPECTRA &&
                  C::kMeans == RH_TC_COUNT,
              "rh_channels.h and rafthip.h agree on the rows and the channel order");

// C(w) of one mode-2 pair: re [nw], im [nw]
extern "C" void rh_chan_control_tf_host(const double* par, const double* dloads6, double z_hub, int nw, const double* w,
                                        double* re, double* im) {
  const A::Derivs d = A::load_derivs(dloads6);
  for (int i = 0; i < nw; ++i) C::control_tf(par, d, z_hub, w[i], re[i], im[i]);
}

// rh_turbine_channels on the host: the same arguments (every pointer a host pointer, the pair columns
// once) and outputs.  Returns 0, or where the entry returns RH_EINVAL for the sizes -1 and for the
// pair columns -(1 + the reason of rh::chan::check_pairs).
extern "C" int rh_turbine_channels_host(int ncase, int nrow, int nw, double dw, const double* w, const double* Xi,
                                        const double* pitch0, int nrot, const double* geom, int npair,
                                        const int* pair_case, const int* pair_rotor, const int* pair_mode,
                                        const double* loads, const double* dloads, const double* param, const double* op,
                                        const double* pair_row, const int* pair_vw, int nvw, const double* V_w,
                                        double* psd, double* stdv, double* avg) {
  if (ncase < 1 || nrow < 1 || nw < 1 || nrot < 1 || nrot > RH_CHAN_MAX_ROTORS || npair < 0 || (npair > 0 && nvw < 1) ||
      !(dw > 0.0))
    return -1;
  int where = 0;
  const int why = npair > 0 ? C::check_pairs(ncase, nrot, npair, nvw, RH_AERO_MAX_PAIRS, pair_case, pair_rotor, pair_mode,
                                             pair_vw, &where)
                            : 0;
  if (why != C::kFine) return -(1 + why);
  for (int c = 0; c < ncase; ++c) {
    const int first = npair > 0 ? A::first_at_least(pair_case, npair, c) : 0;
    const int past = npair > 0 ? A::first_at_least(pair_case, npair, c + 1) : 0;
    const double sp0 = pitch0 ? sin(pitch0[c]) : 0.0;
    for (int ir = 0; ir < nrot; ++ir) {
      const int p = C::pair_of_rotor(pair_rotor, first, past, RH_AERO_MAX_PAIRS, ir);
      const C::Rotor r = C::rotor_of(geom + (long)ir * RH_CG_COUNT, p >= 0 ? param + (long)p * RH_AP_COUNT : nullptr,
                                     p >= 0 ? dloads + (long)p * 6 : nullptr, p >= 0 ? pair_row + (long)p * RH_CP_COUNT : nullptr);
      const double* vrow = r.mode == 2 ? V_w + (long)pair_vw[p] * nw : nullptr;
      C::means(r, sp0, p >= 0 ? loads + (long)p * 8 : nullptr, p >= 0 ? op + (long)p * 5 : nullptr,
               avg + ((long)c * nrot + ir) * RH_TC_COUNT);
      double ss[RH_TC_SPECTRA] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int b = 0; b < nw; ++b) {
        const C::Bin bin = C::bin_of(r, w[b]);
        double pp[RH_TC_SPECTRA] = {0.0, 0.0, 0.0, 0.0, 0.0}, m2[RH_TC_SPECTRA];
        for (int row = 0; row < nrow; ++row) {
          const double* xs = Xi + 2 * ((((long)c * nrow + row) * 6 + 0) * nw + b);
          const double* xp = Xi + 2 * ((((long)c * nrow + row) * 6 + 4) * nw + b);
          C::row_abs2(r, bin, xs[0], xs[1], xp[0], xp[1], m2);
          for (int k = 0; k < RH_TC_SPECTRA; ++k) pp[k] += C::psd_term(m2[k], dw), ss[k] += m2[k];
        }
        if (vrow) {
          C::wind_abs2(r, bin, vrow[b], m2);
          for (int k = RH_TC_OMEGA; k < RH_TC_SPECTRA; ++k) pp[k] += C::psd_term(m2[k], dw), ss[k] += m2[k];
        }
        if (psd)
          for (int k = 0; k < RH_TC_SPECTRA; ++k)
            psd[(((long)c * nrot + ir) * RH_TC_SPECTRA + k) * nw + b] = C::psd_units(k, pp[k]);
      }
      for (int k = 0; k < RH_TC_SPECTRA; ++k)
        stdv[((long)c * nrot + ir) * RH_TC_SPECTRA + k] = C::rms_units(k, sqrt(0.5 * ss[k]));
    }
  }
  return 0;
}

#ifdef CHANNELS_HOST_MAIN
#include <stdio.h>
#include <vector>

static int run_shape(int nw, int nrow, double* checksum) {
  // case 0: rotor 0 mode 2; case 1: no pair; case 2: rotors 0 (mode 1) and 1 (mode 2); case 3: rotor 1 mode 1
  const int ncase = 4, nrot = 2, npair = 4, nvw = 2;
  const int pair_case[npair] = {0, 2, 2, 3}, pair_rotor[npair] = {0, 0, 1, 1}, pair_mode[npair] = {2, 1, 2, 1};
  const int pair_vw[npair] = {1, 0, 0, 1};
  std::vector<double> w(nw), Xi((size_t)ncase * nrow * 6 * nw * 2), pitch0(ncase), geom(nrot * RH_CG_COUNT);
  std::vector<double> loads(npair * 8), dloads(npair * 6), param(npair * RH_AP_COUNT, 0.0), op(npair * 5);
  std::vector<double> prow(npair * RH_CP_COUNT, 0.0), Vw((size_t)nvw * nw);
  for (int i = 0; i < nw; ++i) w[i] = 0.05 * (i + 1), Vw[i] = 2.0 / (1.0 + i), Vw[nw + i] = 0.5 + 0.01 * i;
  for (size_t i = 0; i < Xi.size(); ++i) Xi[i] = 0.01 * (double)((i * 37) % 101) - 0.5;
  for (int c = 0; c < ncase; ++c) pitch0[c] = 0.01 * (c + 1);
  for (int ir = 0; ir < nrot; ++ir) {
    const double g[RH_CG_COUNT] = {150.0 - 10 * ir, 2.2e6, 60.0 + ir, 45.0, 3.1e9, 9.81, 15.0, ir == 0 ? 1.0 : 0.0};
    for (int e = 0; e < RH_CG_COUNT; ++e) geom[ir * RH_CG_COUNT + e] = g[e];
  }
  for (int p = 0; p < npair; ++p) {
    double* par = &param[p * RH_AP_COUNT];
    par[RH_AP_MODE] = pair_mode[p];
    const double cy = cos(0.1 * (p + 1)), sy = sin(0.1 * (p + 1));
    const double Rq[9] = {cy, -sy, 0.0, sy, cy, 0.0, 0.0, 0.0, 1.0};
    for (int e = 0; e < 9; ++e) par[RH_AP_RQ + e] = Rq[e];
    par[RH_AP_RHUB + 0] = -10.0 - p, par[RH_AP_RHUB + 1] = 0.5 * p, par[RH_AP_RHUB + 2] = 150.0;
    par[RH_AP_I_DRIVETRAIN] = 3.2e8, par[RH_AP_NG] = 1.0, par[RH_AP_K_FLOAT] = -9.0;
    par[RH_AP_KP_BETA] = p == 2 ? 0.0 : 0.6, par[RH_AP_KI_BETA] = p == 2 ? 0.0 : 0.1;
    par[RH_AP_KP_TAU] = p == 2 ? -3.8e7 : 0.0, par[RH_AP_KI_TAU] = p == 2 ? -4.6e6 : 0.0;
    prow[p * RH_CP_COUNT + RH_CP_ZHUB] = 150.0, prow[p * RH_CP_COUNT + RH_CP_KP_TAU] = -3.8e7;
    prow[p * RH_CP_COUNT + RH_CP_KI_TAU] = -4.6e6;
    const double L[8] = {1.5e6, 2e3, -1e4, 1.9e7, 4e5, -2e5, 3e7, 1.5e7};
    const double D[6] = {2.1e5, 1.6e5, -1.2e5, 1.5e6, -3.4e6, -1.9e6};
    const double O[5] = {10.0 + p, 7.0, 3.0 * p, 0.1, 0.02};
    for (int e = 0; e < 8; ++e) loads[p * 8 + e] = L[e] * (1.0 + 0.1 * p);
    for (int e = 0; e < 6; ++e) dloads[p * 6 + e] = D[e] * (1.0 - 0.05 * p);
    for (int e = 0; e < 5; ++e) op[p * 5 + e] = O[e];
  }
  const size_t ns = (size_t)ncase * nrot * RH_TC_SPECTRA;
  std::vector<double> psd(ns * nw, -1.0), sd(ns, -1.0), avg((size_t)ncase * nrot * RH_TC_COUNT, -1.0);
  int bad = 0;
  bad += rh_turbine_channels_host(ncase, nrow, nw, 0.05, w.data(), Xi.data(), pitch0.data(), nrot, geom.data(), npair,
                                  pair_case, pair_rotor, pair_mode, loads.data(), dloads.data(), param.data(), op.data(),
                                  prow.data(), pair_vw, nvw, Vw.data(), psd.data(), sd.data(), avg.data()) != 0;
  for (double v : psd) *checksum += v, bad += !(v >= 0.0);
  for (double v : sd) *checksum += v, bad += !(v >= 0.0);
  for (double v : avg) *checksum += v, bad += !(v == v);
  auto S = [&](int c, int ir, int k) { return sd[((size_t)c * nrot + ir) * RH_TC_SPECTRA + k]; };
  bad += !(S(0, 0, RH_TC_OMEGA) > 0.0 && S(0, 0, RH_TC_TORQUE) > 0.0 && S(0, 0, RH_TC_BPITCH) > 0.0);   // mode 2
  bad += !(S(2, 1, RH_TC_OMEGA) > 0.0 && S(2, 1, RH_TC_MBASE) == 0.0);          // mode 2 on a rotor without a tower
  for (int k = RH_TC_OMEGA; k < RH_TC_SPECTRA; ++k)                              // no pair, mode 1: the reference's zeros
    bad += S(1, 0, k) != 0.0 || S(1, 1, k) != 0.0 || S(2, 0, k) != 0.0 || S(3, 1, k) != 0.0;
  bad += !(S(1, 0, RH_TC_MBASE) > 0.0 && S(2, 0, RH_TC_MBASE) > 0.0 && S(1, 0, RH_TC_AXRNA) > 0.0);
  // the same launch without the PSD, and a batch without pairs (null pair tables)
  std::vector<double> sd2(ns, -1.0), avg2(avg.size(), -1.0);
  bad += rh_turbine_channels_host(ncase, nrow, nw, 0.05, w.data(), Xi.data(), pitch0.data(), nrot, geom.data(), npair,
                                  pair_case, pair_rotor, pair_mode, loads.data(), dloads.data(), param.data(), op.data(),
                                  prow.data(), pair_vw, nvw, Vw.data(), nullptr, sd2.data(), avg2.data()) != 0;
  bad += sd2 != sd || avg2 != avg;
  bad += rh_turbine_channels_host(ncase, nrow, nw, 0.05, w.data(), Xi.data(), nullptr, nrot, geom.data(), 0, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                  psd.data(), sd2.data(), avg2.data()) != 0;
  bad += sd2[RH_TC_SPECTRA * nrot + RH_TC_MBASE] != S(1, 0, RH_TC_MBASE) || avg2[RH_TC_AXRNA] != 0.0;
  // refused tables
  auto refused = [&](const int* pc, const int* pr, const int* pm, const int* pv) {
    return rh_turbine_channels_host(ncase, nrow, nw, 0.05, w.data(), Xi.data(), pitch0.data(), nrot, geom.data(), npair, pc,
                                    pr, pm, loads.data(), dloads.data(), param.data(), op.data(), prow.data(), pv, nvw,
                                    Vw.data(), psd.data(), sd2.data(), avg2.data());
  };
  const int dec[npair] = {0, 2, 1, 3}, out_c[npair] = {0, 2, 2, 4}, twice[npair] = {0, 1, 1, 1}, rot9[npair] = {0, 0, 2, 1};
  const int mode3[npair] = {2, 1, 3, 1}, vw2[npair] = {1, 0, 2, 1};
  bad += refused(dec, pair_rotor, pair_mode, pair_vw) != -(1 + C::kCaseDecreases);
  bad += refused(out_c, pair_rotor, pair_mode, pair_vw) != -(1 + C::kCaseRange);
  bad += refused(pair_case, twice, pair_mode, pair_vw) != -(1 + C::kRotorTwice);
  bad += refused(pair_case, rot9, pair_mode, pair_vw) != -(1 + C::kRotorRange);
  bad += refused(pair_case, pair_rotor, mode3, pair_vw) != -(1 + C::kMode);
  bad += refused(pair_case, pair_rotor, pair_mode, vw2) != -(1 + C::kVwRange);
  return bad;
}

int main() {
  int bad = 0;
  double sum = 0.0;
  const int shapes[4][2] = {{1, 1}, {67, 1}, {1, 3}, {67, 3}};
  for (auto& s : shapes) bad += run_shape(s[0], s[1], &sum);
  printf("channels_host: nw 1 and 67, nrow 1 and 3, four cases, two rotors: checksum %.6e, %d failures\n", sum, bad);
  return bad ? 1 : 0;
}
#endif
