// Stand-alone check of the batched entry points' argument errors, for a sanitizer run on the CPU:
// rh_solve_cases, rh_wave_excitation, rh_heading_response and rh_array_solve_stats with no designs, with
// null tables and with designs on different frequency grids, and rh_set_solver / rh_set_qtf_path with the
// values of the removed variant kernels, must each return RH_EINVAL with a message.
// These errors return before the context is read and before any HIP call, so the program needs no GPU:
// the context is an opaque non-null pointer to one byte, which a sanitizer would see any access beyond.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     tools/abi_args_host.cpp raft-teststuff_amd/csrc/rh_abi.hip raft-teststuff_amd/csrc/rh_solve_fast.hip \
//     raft-teststuff_amd/csrc/rh_solve_split.hip -o abi_args_host && ./abi_args_host
#include <cstdio>
#include <cstring>

#include "../include/rafthip.h"

namespace {

int g_bad = 0;

void expect_einval(const char* what, int r) {
  const char* msg = rh_last_error();
  const bool ok = r == RH_EINVAL && msg && std::strlen(msg) > 0;
  std::printf("%-52s -> %d \"%s\"%s\n", what, r, msg ? msg : "(null)", ok ? "" : "   <-- expected RH_EINVAL with a message");
  g_bad += ok ? 0 : 1;
}

}  // namespace

int main() {
  char ctx_byte = 0;
  rh_ctx* ctx = reinterpret_cast<rh_ctx*>(&ctx_byte);
  // stand-ins for device arrays: compared with NULL on the host, never read there
  double dd[1] = {0.0};
  int ii[1] = {0};
  rh_c128 cc[1] = {{0.0, 0.0}};

  rh_design ok;
  std::memset(&ok, 0, sizeof ok);
  ok.nw = 8, ok.nn = 0, ok.nhead = 1, ok.dw = 0.1;
  ok.w = ok.k = ok.M = ok.B = ok.C = dd;
  ok.uhat = ok.finer = ok.kproj = cc;
  rh_design mixed[2] = {ok, ok};
  mixed[1].nw = 16;   // another frequency grid
  rh_design bare = ok;
  bare.uhat = bare.finer = bare.kproj = nullptr;   // no wave tables
  rh_design no_w = ok;
  no_w.w = nullptr;

  rh_cases cases;
  std::memset(&cases, 0, sizeof cases);
  cases.ncase = 1, cases.nIter = 4, cases.XiStart = 0.1, cases.tol = 0.01;
  cases.design = cases.head = cases.spectrum = ii;
  cases.Hs = cases.Tp = cases.gamma = dd;
  rh_solve_out out;
  std::memset(&out, 0, sizeof out);
  out.Xi = out.Xi_last = cc;
  out.iters = out.status = ii;

  expect_einval("rh_solve_cases, ndesign = 0", rh_solve_cases(ctx, &ok, 0, &cases, &out, nullptr));
  expect_einval("rh_solve_cases, designs = NULL", rh_solve_cases(ctx, nullptr, 1, &cases, &out, nullptr));
  expect_einval("rh_solve_cases, no wave tables", rh_solve_cases(ctx, &bare, 1, &cases, &out, nullptr));
  expect_einval("rh_solve_cases, w = NULL", rh_solve_cases(ctx, &no_w, 1, &cases, &out, nullptr));
  expect_einval("rh_solve_cases, mismatched nw", rh_solve_cases(ctx, mixed, 2, &cases, &out, nullptr));

  expect_einval("rh_wave_excitation, ndesign = 0", rh_wave_excitation(ctx, &ok, 0, 1, ii, ii, dd, dd, cc, nullptr));
  expect_einval("rh_wave_excitation, designs = NULL", rh_wave_excitation(ctx, nullptr, 1, 1, ii, ii, dd, dd, cc, nullptr));
  expect_einval("rh_wave_excitation, no wave tables", rh_wave_excitation(ctx, &bare, 1, 1, ii, ii, dd, dd, cc, nullptr));
  expect_einval("rh_wave_excitation, mismatched nw", rh_wave_excitation(ctx, mixed, 2, 1, ii, ii, dd, dd, cc, nullptr));

  expect_einval("rh_heading_response, ndesign = 0", rh_heading_response(ctx, &ok, 0, 1, ii, ii, dd, dd, dd, cc, nullptr));
  expect_einval("rh_heading_response, designs = NULL",
                rh_heading_response(ctx, nullptr, 1, 1, ii, ii, dd, dd, dd, cc, nullptr));
  expect_einval("rh_heading_response, no wave tables", rh_heading_response(ctx, &bare, 1, 1, ii, ii, dd, dd, dd, cc, nullptr));
  expect_einval("rh_heading_response, mismatched nw", rh_heading_response(ctx, mixed, 2, 1, ii, ii, dd, dd, dd, cc, nullptr));

  expect_einval("rh_array_solve_stats, ndesign = 0",
                rh_array_solve_stats(ctx, &ok, 0, 1, 1, ii, dd, nullptr, cc, 0.0, nullptr, nullptr, nullptr));
  expect_einval("rh_array_solve_stats, designs = NULL",
                rh_array_solve_stats(ctx, nullptr, 1, 1, 1, ii, dd, nullptr, cc, 0.0, nullptr, nullptr, nullptr));
  expect_einval("rh_array_solve_stats, w = NULL",
                rh_array_solve_stats(ctx, &no_w, 1, 1, 1, ii, dd, nullptr, cc, 0.0, nullptr, nullptr, nullptr));
  expect_einval("rh_array_solve_stats, mismatched nw",
                rh_array_solve_stats(ctx, mixed, 2, 1, 1, ii, dd, nullptr, cc, 0.0, nullptr, nullptr, nullptr));

  // the selectors of the removed variant kernels (refused before the context is written)
  for (int which = 2; which <= 5; ++which) {
    char what[32];
    std::snprintf(what, sizeof what, "rh_set_solver, which = %d", which);
    expect_einval(what, rh_set_solver(ctx, which));
  }
  expect_einval("rh_set_qtf_path, path = 2", rh_set_qtf_path(ctx, 2));
  expect_einval("rh_set_qtf_path, path = 3", rh_set_qtf_path(ctx, 3));

  std::printf("%s\n", g_bad ? "FAILED" : "all argument errors returned RH_EINVAL with a message");
  return g_bad ? 1 : 0;
}
