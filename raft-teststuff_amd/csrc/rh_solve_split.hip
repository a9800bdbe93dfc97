// rh_solve_split.hip -- the third translation unit of librafthip.so: k_solve_lds<2, 512> (rh_solve.hip)
// compiled once more with one phase-C node sweep per bin, as k_solve_lds_split<2, 512>.
//
// The default two-bin kernel forms the excitation of both bins of a thread in one sweep (kJointC).  This
// is the form before that, kept for two callers: rh_set_solver(ctx, 8 / 9), against which the joint
// sweep is checked bit for bit on one build (tests/test_gpu_joint_phase_c.py), and a call that leaves
// the joint sweep no block to park bin 1's excitation in.  A unit of its own, not a second template
// argument: the kernel's text is then the same function with one constant changed, nothing of either
// form sits in the other's code, and the default kernel keeps its name in profiles and in
// tools/isa_check.py.  Built with rh_solve_fast.hip's flags (__graft_entry__.py UNITS).
#define RH_JOINT_C 0
#define RH_BATCH_B 0   // phase B in its plain form too: the cross-check then covers the default's batched reads
#define k_solve_lds k_solve_lds_split
#include "rh_solve.hip"
#undef k_solve_lds
#include "rh_solve_launch.h"

namespace rh {

hipError_t launch_solve_split(dim3 grid, dim3 block, size_t lsm, hipStream_t s, const CaseArgs& a) {
  hipLaunchKernelGGL((k_solve_lds_split<2>), grid, block, lsm, s, a);
  return hipGetLastError();
}

}  // namespace rh
