// Host build of rh::lu_solve<6> (csrc/rh_device.h) in both forms of its row exchange, for
// tests/test_lu_rows_host.py: ROWS = true, one uniform test per candidate row (every kernel but
// k_solve_cases<2> and <8>), and ROWS = false, one test per step around the chain over every row.
//
// On the device a lane enters a row's block whenever some lane of its wave pivots to that row, so with
// its own `sw` false as often as not.  The host's wave_any has one lane and never does that.  Compiled
// with -DRH_HOST_WAVE_ANY_TRUE it answers true always: every block of every step is entered, as for a
// lane whose wave mates pivot to every row.  The test holds the two builds to the same bits; that
// invariant (a block entered with sw false changes nothing) is what makes the device form safe.
// With -DLU_ROWS_HOST_MAIN it is a stand-alone program over built-in systems (for a sanitizer run on the
// CPU): g++ -O1 -g -fsanitize=address,undefined -DLU_ROWS_HOST_MAIN [-DRH_HOST_WAVE_ANY_TRUE].
#include "../raft-teststuff_amd/csrc/rh_device.h"

namespace {

template <bool ROWS>
void solve_all(int n, const double* A, const double* b, double* x, int* ok) {
  for (int s = 0; s < n; ++s) {
    rh::cd M[6][6], v[6];
    const double* As = A + (long)s * 72;
    const double* bs = b + (long)s * 12;
    for (int i = 0; i < 6; ++i) {
      for (int j = 0; j < 6; ++j) M[i][j] = rh::mk(As[2 * (6 * i + j)], As[2 * (6 * i + j) + 1]);
      v[i] = rh::mk(bs[2 * i], bs[2 * i + 1]);
    }
    ok[s] = rh::lu_solve<6, ROWS>(M, v) ? 1 : 0;
    for (int i = 0; i < 6; ++i) x[(long)s * 12 + 2 * i] = v[i].r, x[(long)s * 12 + 2 * i + 1] = v[i].i;
  }
}

}  // namespace

// n systems: A [n][6][6] and b [n][6] complex (re, im pairs) in, x [n][6] and ok [n] out.  x is what the
// elimination leaves (the kernels store NaN instead wherever ok is 0).
extern "C" void rh_lu_rows6_host(int n, const double* A, const double* b, double* x, int* ok) {
  solve_all<true>(n, A, b, x, ok);
}
extern "C" void rh_lu_chain6_host(int n, const double* A, const double* b, double* x, int* ok) {
  solve_all<false>(n, A, b, x, ok);
}
// 1 if this build enters every block (RH_HOST_WAVE_ANY_TRUE), so that the test knows which build it holds
extern "C" int rh_lu_rows_enters_all() { return rh::wave_any(false) ? 1 : 0; }

#ifdef LU_ROWS_HOST_MAIN
#include <stdio.h>
#include <string.h>

// A dominant matrix as it stands, with its rows reversed, rotated by one (an exchange at every step) and
// with a zero column, through both forms: the same bytes from both, the verdicts 1, 1, 1, 0.
int main() {
  double A[4][72], b[4][12], x[2][4][12];
  int ok[2][4];
  const int rot[6] = {1, 2, 3, 4, 5, 0};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const double re = (i == j ? 4.0 : 0.0) + 0.1 * ((7 * i + 3 * j) % 5 - 2), im = 0.1 * ((5 * i + 2 * j) % 7 - 3);
      A[0][2 * (6 * i + j)] = re, A[0][2 * (6 * i + j) + 1] = im;
      A[1][2 * (6 * (5 - i) + j)] = re, A[1][2 * (6 * (5 - i) + j) + 1] = im;
      A[2][2 * (6 * rot[i] + j)] = re, A[2][2 * (6 * rot[i] + j) + 1] = im;
      A[3][2 * (6 * i + j)] = j == 2 ? 0.0 : re, A[3][2 * (6 * i + j) + 1] = j == 2 ? 0.0 : im;
    }
  for (int s = 0; s < 4; ++s)
    for (int i = 0; i < 6; ++i) b[s][2 * i] = 1.0 + i, b[s][2 * i + 1] = 0.5 - s;
  rh_lu_rows6_host(4, &A[0][0], &b[0][0], &x[0][0][0], ok[0]);
  rh_lu_chain6_host(4, &A[0][0], &b[0][0], &x[1][0][0], ok[1]);
  int bad = 0;
  bad += memcmp(x[0], x[1], sizeof x[0]) != 0;
  for (int f = 0; f < 2; ++f) bad += !(ok[f][0] == 1 && ok[f][1] == 1 && ok[f][2] == 1 && ok[f][3] == 0);
  printf("lu_rows_host: enters every block %d, x[1][0] = %.17g %+.17gi, %s\n", rh_lu_rows_enters_all(), x[0][1][0],
         x[0][1][1], bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
