// Host build of the dense complex solves of csrc/rh_device.h for the CPU check against mpmath
// (tests/test_lu_fma_host.py): rh::lu_solve<6> and rh::lu_factor<6> / rh::lu_apply<6> as the kernels
// instantiate them, one system after the other instead of one per lane.
// With -DLU_HOST_MAIN it is a stand-alone program that runs built-in systems through the exchange, the
// no-exchange and the zero-pivot branches (for a sanitizer run on the CPU):
// g++ -O1 -g -fsanitize=address,undefined -DLU_HOST_MAIN.
#include "../raft-teststuff_amd/csrc/rh_device.h"

namespace {

void load(const double* A, const double* b, rh::cd (&M)[6][6], rh::cd (&x)[6]) {
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) M[i][j] = rh::mk(A[2 * (6 * i + j)], A[2 * (6 * i + j) + 1]);
    x[i] = rh::mk(b[2 * i], b[2 * i + 1]);
  }
}

void store(const rh::cd (&x)[6], double* out) {
  for (int i = 0; i < 6; ++i) out[2 * i] = x[i].r, out[2 * i + 1] = x[i].i;
}

}  // namespace

// n systems: A [n][6][6] and b [n][6] complex (re, im pairs) in, x [n][6] and ok [n] out.  x is what the
// elimination leaves (the kernels store NaN instead wherever ok is 0).
extern "C" void rh_lu_solve6_host(int n, const double* A, const double* b, double* x, int* ok) {
  for (int s = 0; s < n; ++s) {
    rh::cd M[6][6], v[6];
    load(A + (long)s * 72, b + (long)s * 12, M, v);
    ok[s] = rh::lu_solve<6>(M, v) ? 1 : 0;
    store(v, x + (long)s * 12);
  }
}

// The same systems through lu_factor<6> and lu_apply<6>: after a zero pivot every row of x is NaN.
extern "C" void rh_lu_factor_apply6_host(int n, const double* A, const double* b, double* x, int* ok) {
  for (int s = 0; s < n; ++s) {
    rh::cd M[6][6], v[6];
    int piv[6];
    load(A + (long)s * 72, b + (long)s * 12, M, v);
    ok[s] = rh::lu_factor<6>(M, piv) ? 1 : 0;
    rh::lu_apply<6>(M, piv, v);
    store(v, x + (long)s * 12);
  }
}

#ifdef LU_HOST_MAIN
#include <stdio.h>

// A dominant matrix as it stands (no exchange), with its rows reversed (exchanges at steps 0, 1, 2) and
// with a zero column (a zero pivot at step 2), each through both entry points.
int main() {
  double A[3][72], b[3][12], x[3][12];
  int ok[3];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const double re = (i == j ? 4.0 : 0.0) + 0.1 * ((7 * i + 3 * j) % 5 - 2), im = 0.1 * ((5 * i + 2 * j) % 7 - 3);
      A[0][2 * (6 * i + j)] = re, A[0][2 * (6 * i + j) + 1] = im;
      A[1][2 * (6 * (5 - i) + j)] = re, A[1][2 * (6 * (5 - i) + j) + 1] = im;
      A[2][2 * (6 * i + j)] = j == 2 ? 0.0 : re, A[2][2 * (6 * i + j) + 1] = j == 2 ? 0.0 : im;
    }
  for (int s = 0; s < 3; ++s)
    for (int i = 0; i < 6; ++i) b[s][2 * i] = 1.0 + i, b[s][2 * i + 1] = 0.5 - s;
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    (pass ? rh_lu_factor_apply6_host : rh_lu_solve6_host)(3, &A[0][0], &b[0][0], &x[0][0], ok);
    bad += !(ok[0] == 1 && ok[1] == 1 && ok[2] == 0);
    for (int s = 0; s < 2; ++s) {   // the residual of the two regular systems
      double worst = 0.0;
      for (int i = 0; i < 6; ++i) {
        double rr = b[s][2 * i], ri = b[s][2 * i + 1];
        for (int j = 0; j < 6; ++j) {
          const double ar = A[s][2 * (6 * i + j)], ai = A[s][2 * (6 * i + j) + 1];
          rr -= ar * x[s][2 * j] - ai * x[s][2 * j + 1];
          ri -= ar * x[s][2 * j + 1] + ai * x[s][2 * j];
        }
        worst = fmax(worst, fmax(fabs(rr), fabs(ri)));
      }
      bad += !(worst < 1e-13);
      printf("lu_host: pass %d system %d residual %.2e\n", pass, s, worst);
    }
    if (pass) bad += !(x[2][0] != x[2][0]);   // lu_apply after a zero pivot: NaN
  }
  return bad ? 1 : 0;
}
#endif
