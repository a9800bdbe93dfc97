// rh_solve.hip -- k_solve_lds: the per-case drag fixed point with the relaxed iterate in LDS.
//
// Same algorithm and arithmetic as k_solve_cases (rh_kernels.hip; raft/raft_model.py:918-1000,
// raft/raft_fowt.py:1152-1293), re-laid-out for latency on gfx950:
//   * 512 threads (8 waves) per case, one case per CU; lane = bin, NB <= 2 bins per thread.
//   * XiLast lives in LDS ([6][512 NB] complex) for the whole solve: the thread that owns a
//     bin is the only one that reads or writes it, so no global round trip per iteration.
//     The unrelaxed solution is streamed to HBM with non-temporal stores (it is only
//     consumed after the loop), so it does not evict the wave tables from L2.
//   * The projected wave table (kproj, the only per-node stream) is read through a buffer
//     resource (one 32-bit lane offset per bin, node/projection offsets scalar) with a register
//     ring of kRingA1 / kRingC nodes (the two transverse rows of each).  The node loops run whole
//     ring rounds with no load under a branch, so that every wait leaves the other slots' loads
//     outstanding (tools/isa_check.py gates it).
//   * Per-node bin sums: transposing wave reductions of several sums at once (tbfly8 / tbfly4 /
//     tbfly3: the rows first, two values per gfx950 row swap, then DPP inside the row; VALU only,
//     no LDS or SGPR traffic), one partial per wave, summed in wave order.  Every sum meets the
//     same partners in the same order whichever slot it is in, so results are deterministic and
//     do not depend on how nodes are grouped.
//   * The axial row of a node (projection 0) is read only where the node has axial side drag or
//     end drag, in short loops of their own after the node loops of phases A and C; elsewhere it
//     would meet coefficients that are exact zeros.
#include "rh_common.h"

namespace rh {

#ifdef RH_PROF
// Phase cycle counters (s_memtime of wave 0 of every workgroup), summed over workgroups:
// [0] prologue [1] A [2] B [3] C excitation [4] C solve [5] flags [6] epilogue [7] iterations
static __device__ unsigned long long rh_prof[12];   // static: one per translation unit (rh_prof_read reads rh_solve_fast.hip's)
#define PROF_T(v) const unsigned long long v = clock64()
#define PROF_ADD(i, x) if (tid == 0) atomicAdd(&rh_prof[i], (unsigned long long)(x))
#else
#define PROF_T(v)
#define PROF_ADD(i, x)
#endif

#ifdef RH_WGTIME
// Per-workgroup wall-clock (s_memrealtime, 100 MHz) of the fixed point: [2 slot] = start,
// [2 slot + 1] = end of the loop, by dispatch slot (launch-tail analysis, tools/ubench/wg_times.py)
static __device__ unsigned long long rh_wgt[2 * 8192];
#endif

constexpr int kLT = 512;          // threads per case workgroup
constexpr int kLW = kLT / 64;     // waves per case workgroup
#ifndef RH_RING_A
#define RH_RING_A 4               // (3 in the two-pass kernel: 4 moves its spills into the streaming loops)
#endif
#ifndef RH_RING_C
#define RH_RING_C 6
#endif
constexpr int kRingA1 = RH_RING_A; // wave-table prefetch depth (nodes) of phase A
constexpr int kRingC = RH_RING_C; // ... of phase C (one bin per pass: less work per node)
constexpr int kAxC = 4;               // axial wave-table rows phase C holds at a time (its own path, beside the ring)
#ifndef RH_JOINT_C
#define RH_JOINT_C 1                  // 1: k_solve_lds<2, 512> forms both bins' excitation in one phase-C node sweep
#endif
constexpr bool kJointC = RH_JOINT_C != 0;
#ifndef RH_BATCH_B
#define RH_BATCH_B 1                  // 1: phase B reads its LDS operands in batches ahead of their uses; 0: one by one (A/B)
#endif
// The joint sweep's ring: the kRingC slots hold one (node, bin) each, so it is kRingC / 2 nodes deep
// with the same rows in flight (and the same registers) as the one-bin ring.
constexpr int kRingCJ = kRingC / 2;
static_assert(kRingC % 2 == 0, "the joint phase-C ring pairs its slots");
// Ghost nodes: the node loops of phases A and C run whole ring rounds, so no slot of a round is
// under a tail guard (a guarded slot is a merge point at which hipcc stops counting the ring's loads
// and waits for all of them).  Nodes nn .. of the last round load the last node's rows
// again and meet zero coefficients in phase C (exact +0) or write no partial in phase A.  The
// node-indexed LDS tables that the loops read carry one zero row, row nn, for all of them (56
// bytes: the C4 kernel's four workgroups per CU have about 300 bytes of LDS to spare).
constexpr int kGhost = 1;

// |a|^2 as fma(re, re, im im), said outright.  Left to the compiler (abs2), which of the two products is
// fused follows from the order of the sum's operands in its graph, and an unrelated change in phase B
// swapped it in the PSD and RMS sums of the rotations ("Phase B's LDS chains").
__device__ __forceinline__ double abs2_re(cd a) { return __builtin_fma(a.r, a.r, a.i * a.i); }

// A scalar zero the compiler cannot fold (see its use in phase C).
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

// The lane index, recomputed where it is used: a hoisted copy would be one more value kept
// live across the whole solve (and spilled, and its reload would drain the prefetch ring,
// since scratch loads share the vector-memory counter with the wave-table loads).
__device__ __forceinline__ int lane_here() {
  int r;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(r));
  return r;
}

template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {   // full-mask permutations: every lane valid
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Pair sums across the rows with the gfx950 row-swap instructions (v_permlane32_swap /
// v_permlane16_swap: VALU, no LDS round trip as with ds_bpermute), two values per exchange.
// v_permlane32_swap x, y exchanges the upper half of x with the lower half of y, so lane L of the
// lower half is left with {x_L, x_(L^32)} and lane L of the upper half with {y_(L^32), y_L}: one add
// gives the lower half x + x(lane ^ 32) and the upper half y + y(lane ^ 32), with no select and no
// copy (FP addition commutes, so both lanes of a pair hold the same bits).  v_permlane16_swap does
// the same with the odd rows of x and the even rows of y: even rows x + x(lane ^ 16), odd rows
// y + y(lane ^ 16).  Call with every lane active.
__device__ __forceinline__ double pair_sum32(double x, double y) {
  const auto a = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}
__device__ __forceinline__ double pair_sum16(double x, double y) {
  const auto a = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
  return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
}

// Transposing wave reductions: several per-lane values in, each lane out with the wave total (all 64
// lanes) of one of them.  The cross-row exchanges come first, where the most values are, because a row
// swap transposes a pair of values in 3 instructions (pair_sum32 / pair_sum16) where an in-row DPP
// stage takes 7 (two selects, two moves, one add):
//   tbfly8  ^32 on (u[p], u[p+4]), ^16 on (v[p], v[p+2]), one transposing DPP stage ^2, plain ^15, ^1, ^7
//   tbfly4  ^32 on (a, c) and (b, d), ^16 on the two results, plain ^2, ^15, ^1, ^7: no select at all
//   tbfly3  tbfly4 with the pad slot 0.0
// (^1 quad_perm [1,0,3,2], ^2 quad_perm [2,3,0,1], ^7 row_half_mirror, ^15 row_mirror.)  Every value
// meets its partners ^32, ^16, ^2, ^15, ^1, ^7 in that order whichever slot and whichever of the three it
// is in, and every add is commutative, so a wave sum's bits do not depend on how the values are
// grouped (tests/test_bfly_model.py is the order written out; the cross-mode tests rely on it).
// The in-row order is one of many of equal cost and equal error bound; DESIGN.md §5 says why this one.
//
// tbfly4 / tbfly3: row r of the wave ends with value r (0 = a .. 3 = d or the pad), every lane of
// the row with the same bits.  One writer per value: lanes 0, 16, 32, 48.
__device__ __forceinline__ double tbfly4(double a, double b, double c, double d) {
  double t = pair_sum16(pair_sum32(a, c), pair_sum32(b, d));
  t += dpp_mov<0x4E>(t);
  t += dpp_mov<0x140>(t);
  t += dpp_mov<0xB1>(t);
  t += dpp_mov<0x141>(t);
  return t;
}
__device__ __forceinline__ double tbfly3(double a, double b, double c) { return tbfly4(a, b, c, 0.0); }
// value a writer lane holds after tbfly4 (0 .. 3) / tbfly3 (0 .. 2), -1 for every other lane
__device__ __forceinline__ int tbfly4_index(int lane) { return (lane & 15) == 0 ? lane >> 4 : -1; }
__device__ __forceinline__ int tbfly3_index(int lane) { return (lane & 15) == 0 && lane < 48 ? lane >> 4 : -1; }

// tbfly8: eight wave sums at once (the transverse sums of a phase-A ring round's four nodes).  After the
// two row stages a lane holds two values; the stage ^2 keeps one of them by the flag f0 = b1 ^ b2 (bits
// of the lane), which differs across ^2 and agrees across ^15, ^1 and ^7, so that the three plain adds
// meet lanes that hold the same value.  A lane ends with value 4 (lane >> 5) + 2 ((lane >> 4) & 1) + f0.
// One writer per value: the lanes with (lane & 13) == 0 (0, 2, 16, 18, 32, 34, 48, 50), where f0 is
// bit 1.  10 exchanges.
struct Bfly4 {   // a lane's stage flag and the values it writes (formed once per phase A)
  bool f0;
  int vi;        // (tbfly4) 0 = a .. 3 = d, or -1 (not a writer lane)
  int vi8;       // (tbfly8) 0 .. 7, or -1
};
__device__ __forceinline__ Bfly4 bfly4_lane(int lane) {
  Bfly4 b;
  b.f0 = (((lane >> 1) ^ (lane >> 2)) & 1) != 0;
  b.vi = tbfly4_index(lane);
  b.vi8 = (lane & 13) != 0 ? -1 : 4 * (lane >> 5) + 2 * ((lane >> 4) & 1) + ((lane >> 1) & 1);
  return b;
}
__device__ __forceinline__ double tbfly8(const double (&u)[8], const Bfly4& L) {
  const bool f0 = L.f0;
  double v[4], w[2];
#pragma unroll
  for (int p = 0; p < 4; ++p) v[p] = pair_sum32(u[p], u[p + 4]);
#pragma unroll
  for (int p = 0; p < 2; ++p) w[p] = pair_sum16(v[p], v[p + 2]);
  double t = (f0 ? w[1] : w[0]) + dpp_mov<0x4E>(f0 ? w[0] : w[1]);
  t += dpp_mov<0x140>(t);
  t += dpp_mov<0xB1>(t);
  t += dpp_mov<0x141>(t);
  return t;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_mov_rows(double v) {   // rows outside ROWS receive 0
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xF, false);
  return __hiloint2double(hi, lo);
}

// Sum over the whole wave, complete in lane 63 only.  Call with every lane active.
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and row_mirror give every lane
// its 16-lane row total r_k; row_bcast:15 then adds r0 into row 1 and r2 into row 3, and
// row_bcast:31 adds row 1 into row 3: lane 63 = (r3 + r2) + (r1 + r0).  VALU only, no
// LDS or SGPR traffic, fixed order.
__device__ __forceinline__ double wave_sum63(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  v += dpp_mov_rows<0x142, 0xA>(v);
  v += dpp_mov_rows<0x143, 0xC>(v);
  return v;
}

// One entry of translateMatrix3to6DOF by block: 0 = Bm[r][c], 1 = (Bm H)[r][c] (the upper-right
// block; the lower-left one is its transpose), 2 = (H Bm H^T)[r][c]; the expressions of t3to6
// (rh_kernels.hip), evaluated for all three and selected, so no lane branches.
__device__ __forceinline__ double t3to6_block(const double* Bm, double rx, double ry, double rz, int blk, int r, int c) {
  const double H[3][3] = {{0, rz, -ry}, {-rz, 0, rx}, {ry, -rx, 0}};
  double hc[3], hr[3];   // column c of H, row r of H (selected without dynamic register indexing)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    hc[k] = c == 0 ? H[k][0] : c == 1 ? H[k][1] : H[k][2];
    hr[k] = r == 0 ? H[0][k] : r == 1 ? H[1][k] : H[2][k];
  }
  double hcc[3];   // row c of H
#pragma unroll
  for (int k = 0; k < 3; ++k) hcc[k] = c == 0 ? H[0][k] : c == 1 ? H[1][k] : H[2][k];
  const double b0 = Bm[3 * r + c];
  const double b1 = Bm[3 * r + 0] * hc[0] + Bm[3 * r + 1] * hc[1] + Bm[3 * r + 2] * hc[2];
  double b2 = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double HB = hr[0] * Bm[0 * 3 + k] + hr[1] * Bm[1 * 3 + k] + hr[2] * Bm[2 * 3 + k];
    b2 += HB * hcc[k];
  }
  return blk == 0 ? b0 : blk == 1 ? b1 : b2;
}

// Entry (i, j) of translateMatrix3to6DOF(Bm, r), t3to6's sums (rh_common.h) with every multiply-add said
// outright, for phase B's entries from a node's Bmat in registers.  Written as sums of products, which
// product of a·b + c·d the compiler fuses follows from how many uses each has, and with one set of nine
// values for all 36 entries the entries share products: other roundings than those of the entries
// formed one by one from the LDS row.  These are the multiply-adds of that form, read from its assembly
// ("Phase B's LDS chains"): the minuend of a difference is the fused product, else the
// first one.  One exception is kept for the bits: (H Bm)[2][1] had its other product fused in the entries
// (5, 3) and (5, 4), where the product was shared with a neighbour (`alt`).
__device__ __forceinline__ double t3to6_fma(const double (&B)[9], double rx, double ry, double rz, int i, int j) {
  auto fma = [](double a, double b, double c) { return __builtin_fma(a, b, c); };
  auto bh = [&](int a, int c) {   // (Bm H)[a][c], H = [[0, rz, -ry], [-rz, 0, rx], [ry, -rx, 0]]
    const double b0 = B[3 * a], b1 = B[3 * a + 1], b2 = B[3 * a + 2];
    return c == 0 ? fma(b2, ry, fma(b0, 0.0, -(b1 * rz)))
         : c == 1 ? fma(b2, -rx, fma(b0, rz, b1 * 0.0))
                  : fma(b2, 0.0, fma(b1, rx, -(b0 * ry)));
  };
  auto hb = [&](int a, int k, bool alt) {   // (H Bm)[a][k]
    const double b0 = B[k], b1 = B[3 + k], b2 = B[6 + k];
    return a == 0 ? fma(-ry, b2, fma(0.0, b0, b1 * rz))
         : a == 1 ? fma(rx, b2, fma(0.0, b1, -(b0 * rz)))
                  : fma(0.0, b2, alt ? fma(-b1, rx, b0 * ry) : fma(b0, ry, -(b1 * rx)));
  };
  if (i < 3 && j < 3) return B[3 * i + j];
  if (i < 3) return bh(i, j - 3);
  if (j < 3) return bh(j, i - 3);
  const int a = i - 3, c = j - 3;   // (H Bm H^T)[a][c] = sum_k (H Bm)[a][k] H[c][k], from 0 in k order
  const double h0 = c == 0 ? 0.0 : c == 1 ? -rz : ry, h1 = c == 0 ? rz : c == 1 ? 0.0 : -rx;
  const double h2 = c == 0 ? -ry : c == 1 ? rx : 0.0;
  return fma(hb(a, 2, false), h2, fma(hb(a, 1, a == 2 && c < 2), h1, fma(hb(a, 0, false), h0, 0.0)));
}

// Every table the loops read is staged here: a global load inside the node loops would share
// the vector-memory counter with the prefetched wave-table loads and force them to drain.
__host__ __device__ inline size_t solve_lds_smem(int nn, int nm, int NB, int LT = kLT, bool ser = false, int NP = 1) {
  const int LW = LT / 64;
  return sizeof(double) * ((size_t)(NP == 1 ? 12 * LT * NB : 0)   // XiLast [6][512 NB] complex (one pass)
                           + (size_t)(ser && nn * 3 * LW < 27 ? 27 : nn * 3 * LW)   // per-wave node sums (SER: >= 27 entries)
                           + (ser ? (size_t)0 : (size_t)nn * 36)   // per-node B_drag contributions
                           + (size_t)nn * 9           // Bmat
                           + (size_t)(nn + kGhost) * 6   // member-factored drag coefficients (stride 6: 16-B rows; ghost row)
                           + (size_t)(nn + kGhost)    // node axial coordinate t
                           + (size_t)nm * 18          // member cq, c1, c2
                           + (size_t)2 * LT * NB * NP   // w and zeta per (padded) bin
                           + 36 + 108 + LW * 6 + 36  // B_drag, M|B|C image, std partials, B_lin+B_drag
                           + LW)                     // convergence-margin partials
         + sizeof(int) * ((size_t)nm + 6);            // member node ranges, vote words, wave counters
}

// LT threads per case: 512 (8 waves), or 256 for nw <= 256 (two cases per CU; C4 has 240 bins),
// or 128 (SER: four cases per CU, B_drag summed node-serially per entry instead of through a
// per-node LDS image, so a workgroup needs about 40 KB of LDS).
// NP > 1 (grids beyond LT NB bins, nw <= 2048): the bins are taken in NP passes of LT NB, and
// XiLast ([6][nw] complex, 192 KB at nw = 2048) no longer fits the LDS: it lives in the case's
// Xi_last block, read and written only by the thread that owns the bin.  Phase A loads a pass's
// XiLast into registers before its node loop (no global load between the ring's wave-table
// loads) and adds each pass's node sums to the LDS partials in pass order; phase C reads and
// writes it around each bin's solve.
//
// JC (joint phase C; kJointC above): one sweep of the phase-C node loop forms the excitation of both
// bins of a thread, in the 512-thread, two-bin, one-pass kernel.  rh_solve_split.hip compiles this
// file once more with RH_JOINT_C = 0 and the kernel renamed k_solve_lds_split: the same fixed point
// with one sweep per bin (rh_set_solver(ctx, 8), and calls that leave no block to park bin 1's
// excitation in).
template <int NB, int LT = kLT, bool SER = false, int NP = 1>
__global__ __launch_bounds__(LT, LT >= 256 ? 512 / LT : 2) void k_solve_lds(CaseArgs a) {
  constexpr bool JC = kJointC && NB == 2 && LT == kLT && !SER && NP == 1;
  constexpr int LW = LT / 64;
  // Phase B with its LDS operands read ahead of their uses: a node's wave partials, its Bmat (kept in
  // registers for the translate entries) and the node sum of B_drag (the non-SER kernels; the SER kernel
  // keeps its own forms)
  constexpr bool kBatchS = RH_BATCH_B != 0 && !SER;
  constexpr int kSumB = 16;                        // per-node B_drag entries read per batch of phase B's node sum
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wv_s = __builtin_amdgcn_readfirstlane(wv);   // wave index in an SGPR
  PROF_T(tp0);
#ifdef RH_WGTIME
  const unsigned long long wgt0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int slot = xcd_remap(blockIdx.x, a.c.ncase);
  const int ic = a.c.order ? a.c.order[slot] : slot;
  const rh_design& d = a.designs[a.c.design[ic]].d;
  const int nw = d.nw, nn = d.nn, nm = d.nm;
  const unsigned nw16 = (unsigned)nw * 16u;
  const double* __restrict__ node = d.node;
  const int head = a.c.head[ic];
  const size_t c6 = (size_t)ic * 6 * nw;
  const Buf bK = mkbuf(d.kproj + (size_t)head * nn * 3 * nw, (unsigned)nn * 3u * nw16);
  const Buf bFe = mkbuf(d.finer + (size_t)head * 6 * nw, 6u * nw16);
  const bool has_fx = a.c.fext != nullptr;
  const Buf bFx = mkbuf(has_fx ? a.c.fext + c6 : nullptr, has_fx ? 6u * nw16 : 0u);

  constexpr int NWP = LT * NB;                    // padded bins of one pass
  constexpr int NBT = NB * NP;                     // bins per thread over all passes
  constexpr bool GX = NP > 1;                      // XiLast in the Xi_last block, not in LDS
  constexpr int kRingA = GX ? 3 : kRingA1;
  // PSD / RAO / RMS sums formed in phase C, where it stores Xi (no read-back), by the 512-thread
  // kernels; the SER kernels (C4's fixed point: no response output) keep them in the epilogue
  constexpr bool kStatsC = !SER && NB > 1;
  constexpr bool kOv = !GX;                        // the vote deferred into the next phase A (below)
  auto wave_maxes = [&](const double* m) {         // max of the per-wave convergence-margin partials
    double mx = m[0];
    for (int w = 1; w < LW; ++w) mx = fmax(mx, m[w]);
    return mx;
  };
  cd* xl = reinterpret_cast<cd*>(smem);            // [6][NWP] (one pass only)
  rh_c128* XL = a.o.Xi_last + c6;                  // [6][nw] (GX)
  // The member factors and the node coefficients, read at every member change and node step of
  // the loops, come first, member- / node-major with 16-byte rows (a member's 18 factors are
  // 9 ds_read_b128 at one base address instead of 18 scattered reads at nm-strided addresses).
  double* mbf = smem + (GX ? 0 : 12 * NWP);        // [nm][18] cq, c1, c2
  double* al = mbf + 18 * nm;                      // [nn + kGhost][6] (5 used; the ghost row stays 0)
  double* red = al + 6 * (nn + kGhost);            // [nn*3][LW]
  double* bm = red + (SER && nn * 3 * LW < 27 ? 27 : nn * 3 * LW);   // [nn][9]
  double* bd = bm + nn * 9;                        // [36]
  double* mbc = bd + 36;                           // [108] M, B_lin, C
  double* sred = mbc + 108;                        // [LW][6]
  double* bsum = sred + LW * 6;                   // [36] B_lin + B_drag of this iteration
  double* bdn = bsum + 36;                         // [36][nn] (not with SER)
  double* nt = bdn + (SER ? 0 : 36 * nn);          // [nn + kGhost] (ghost entry 0)
  double* lw = nt + nn + kGhost;                   // [NP NWP] w per bin (pad bins: w[nw-1])
  double* lz = lw + NP * NWP;                      // [NP NWP] zeta per bin (pad bins: 0)
  double* mred = lz + NP * NWP;                    // [LW] per-wave max of tolCheck
  int* mstart = reinterpret_cast<int*>(mred + LW);  // [nm+1]
  // Which nodes need their axial wave-table row (projection 0): those with axial side drag or
  // end drag, AQ CDQ != 0 or AEND CDEND != 0 (node_bmat_f); for every other node the row enters
  // the result only through coefficients that are exact zeros (Cd_q defaults to 0 and end areas
  // are non-zero only at member ends and diameter steps: 4 of 53 nodes of C2).  Kept in the
  // spare sixth double of the node's `al` row as two ints: [0] the node's flag (phase B), [1] entry
  // k = n of the compact, node-ordered list of the axial nodes (-1 past its end), which the axial
  // loops of phases A and C walk.
  int* ax = reinterpret_cast<int*>(al);
  auto ax_node = [&](int k) { return k < nn ? __builtin_amdgcn_readfirstlane(ax[12 * k + 11]) : -1; };   // k uniform
  int* sflag = mstart + nm + 1;                      // [2] vote words of even / odd iterations,
                                                     // [2]: it + 1 once a test of iteration it failed,
                                                     // [3 + (it & 1)]: waves done with phase C of iteration it
  load_mbc(d, mbc, tid);
  for (int n = tid; n < nn; n += LT) nt[n] = node[RH_NF_T * nn + n];
  // The flags and the list, by wave 0 alone, 64 nodes at a time: the chunk's flags as a ballot, a node's
  // rank as the axial nodes of earlier chunks plus the flags below its lane.  One wave's LDS writes stay
  // in order and the list's entries (k < count) and its padding (k >= count) are different words, so
  // the barrier that ends the prologue is the only one this needs.
  if (wv_s == 0) {
    int nq = 0;   // uniform: axial nodes so far
    for (int n0 = 0; n0 < nn; n0 += 64) {
      const int n = n0 + lane, nc = n < nn ? n : nn - 1;
      const double aq = node[RH_NF_AQ * nn + nc], cdq = node[RH_NF_CDQ * nn + nc];
      const double ae = node[RH_NF_AEND * nn + nc], cde = node[RH_NF_CDEND * nn + nc];
      const bool f = n < nn && (a.all_axial || aq * cdq != 0.0 || ae * cde != 0.0);
      const unsigned long long mask = __ballot(f);
      const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      if (n < nn) ax[12 * n + 10] = f ? 1 : 0;
      if (f) ax[12 * (nq + below) + 11] = n;
      nq += __popcll(mask);
    }
    for (int k = nq + lane; k < nn; k += 64) ax[12 * k + 11] = -1;
  }
  for (int e = tid; e < 18 * nm; e += LT) mbf[e] = d.memb[(e % 18) * nm + e / 18];   // RH_MF_CQ0..C20: fields 0..17
  // (the last member's end is never met by a node index: ghost nodes open or close no member)
  for (int e = tid; e <= nm; e += LT) mstart[e] = e < nm ? d.mstart[e] : INT_MAX;
  for (int e = tid; e < 6 * kGhost; e += LT) al[6 * nn + e] = 0.0;
  for (int e = tid; e < kGhost; e += LT) nt[nn + e] = 0.0;
  if (tid < 5) sflag[tid] = 0;
  const int it0 = a.c.first_iter;

  // Per-bin scalars live in LDS, not in registers: nothing per-thread stays live across the
  // phases, so the register-heavy solve of phase C does not push other values to scratch.
  // Bin j of this thread is b = tid + LT j; loads use the clamped bin min(b, nw-1) so no
  // load is predicated, and pad bins (b >= nw) carry zeta = 0 and XiLast = 0.
  auto voff = [&](int b) { return (unsigned)(b < nw ? b : nw - 1) * 16u; };
  {
    const int spec = a.c.spectrum[ic];
    const double Hs = a.c.Hs[ic], Tp = a.c.Tp[ic], gam = a.c.gamma[ic];
    const rh_c128* XI0 = a.c.Xi_init ? a.c.Xi_init + c6 : nullptr;
    // (the loads first, then the spectrum from LDS: a loop that both loads and evaluates the
    // spectrum's transcendentals keeps scratch stores beside its loads under the max-ilp scheduler)
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int b = tid + LT * j;
      const bool okb = b < nw;
      lw[b] = d.w[okb ? b : nw - 1];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const cd x0 = okb ? (XI0 ? ld(XI0 + c * nw + b) : mk(a.c.XiStart, 0.0)) : mk(0.0, 0.0);
        if constexpr (GX) {
          if (okb) st(XL + c * nw + b, x0);
        } else {
          xl[c * NWP + b] = x0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NBT; ++j) {   // the thread reads back only its own bins: no barrier
      const int b = tid + LT * j;
      const bool okb = b < nw;
      const double zz = sea_amplitude(spec, Hs, Tp, gam, lw[b], d.dw);
      lz[b] = okb ? zz : 0.0;
      if (okb && a.o.zeta) a.o.zeta[(size_t)ic * nw + b] = zz;
    }
  }
  rh_c128* Xo = a.o.Xi ? a.o.Xi + c6 : nullptr;   // NULL: the caller wants no response (C4 fixed point)
  rh_c128* XP = a.o.Xi_prev ? a.o.Xi_prev + c6 : nullptr;
  const double rho = d.rho;
  const int nloop = a.c.nIter + 1;
  const double tol = a.c.tol;
  int status = RH_CASE_NOT_CONVERGED, iters = nloop;
  double margin = INFINITY;   // closest call of the convergence test (rh_solve_out.margin)
  __syncthreads();
  PROF_T(tp1);
  PROF_ADD(0, tp1 - tp0);

  // The excitation of bin j of this thread with the current node coefficients (al, written by
  // phase B), member-factored (drag_exc_members' arithmetic):
  //   f_n = Bmat_n uhat_n = aq q Kq + a1 p1 K1 + a2 p2 K2,  r_n x f_n = rA x f_n + t q x f_n
  // with q x p1 = p2, q x p2 = -p1 (raft/raft_fowt.py:1255-1259, 1283-1289), then
  // F = zeta (F_iner + F_drag) (+ fext), phase C of every iteration.
  auto excite = [&](int bj, cd (&F)[6]) {
    const unsigned vj = voff(bj);
    const bool okj = bj < nw;
    cd fe[6];   // unit inertial excitation of this bin, in flight during the node loop
#pragma unroll
    for (int c = 0; c < 6; ++c) fe[c] = bld(bFe, vj, c * nw16);
#pragma unroll
    for (int c = 0; c < 6; ++c) F[c] = mk(0, 0);
    {
      cd SQ = mk(0, 0), S1 = mk(0, 0), S2 = mk(0, 0), T1 = mk(0, 0), T2 = mk(0, 0);
      auto load1 = [&](cd (&K)[2], int n) {
        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;
#pragma unroll
        for (int p = 0; p < 2; ++p) K[p] = bld(bK, vj, so + (unsigned)(p + 1) * nw16);
      };
      auto load_axial = [&](cd& Kq, int k) {   // row 0 of the k-th axial node (none past the list)
        const int n = ax_node(k);
        if (n >= 0) Kq = bld(bK, vj, (unsigned)n * 3u * nw16);   // uniform
        else Kq = mk(0.0, 0.0);
      };
      int m = 0, mnext = nn > 0 ? mstart[1] : 0;
      auto fold = [&]() {   // close member m: F += sum of its nodes (as drag_exc_members)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const double c1 = mbf[18 * m + RH_MF_C10 + i], c2 = mbf[18 * m + RH_MF_C20 + i];
          F[i] = add(F[i], add(scl(S1, c1), scl(S2, c2)));
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double p1 = mbf[18 * m + RH_MF_C10 + i], p2 = mbf[18 * m + RH_MF_C20 + i];
          F[3 + i] = add(F[3 + i], sub(scl(T1, p2), scl(T2, p1)));
        }
        S1 = S2 = T1 = T2 = mk(0, 0);
      };
      // The node ring carries the two transverse rows of every node.  The axial rows of the few
      // nodes that need them (ax_node) are summed in a short loop of their own after it, as in phase
      // A: a load under a branch inside the node loop, even a uniform one, is a merge point at which
      // hipcc stops counting the ring's loads and waits for nearly all of them.  The
      // first kAxC axial rows are requested before the ring's, so they have arrived behind the node loop.
      // (Both are requested in ring order, each slot scheduled by itself: the waits of the first round
      // are counted from here, and hipcc takes the smaller of this count and the steady state's.)
      cd KQ[kAxC];
#pragma unroll
      for (int r = 0; r < kAxC; ++r) load_axial(KQ[r], nn > 0 ? r : nn);
      __builtin_amdgcn_sched_barrier(0);
      cd K[kRingC][2];
#pragma unroll
      for (int r = 0; r < kRingC; ++r) {
        load1(K[r], r);
        __builtin_amdgcn_sched_barrier(0);
      }
      // node n's coefficient row is read while node n - 1 is consumed (ghost nodes: row nn, zeros)
      double A1 = al[1], A2 = al[2], A3 = al[3], A4 = al[4];
      auto step = [&](cd (&K)[2], int n) {
        while (n == mnext) {   // uniform: member m ended before node n
          fold();
          ++m;
          mnext = mstart[m + 1];
        }
        const double a1 = A1, a2 = A2, a3 = A3, a4 = A4;
        {
          const double* A = al + 6 * (n + 1 < nn ? n + 1 : nn);
          A1 = A[1]; A2 = A[2]; A3 = A[3]; A4 = A[4];
        }
        S1 = add(S1, scl(K[0], a1));
        S2 = add(S2, scl(K[1], a2));
        T1 = add(T1, scl(K[0], a3));
        T2 = add(T2, scl(K[1], a4));
        __builtin_amdgcn_sched_barrier(0);   // consumed before the refill is issued (as in phase A)
        load1(K, n + kRingC);
        __builtin_amdgcn_sched_barrier(0);
      };
#pragma unroll 1
      for (int n = 0; n < nn; n += kRingC) {   // whole rounds: the last one ends in ghost nodes
#pragma unroll
        for (int r = 0; r < kRingC; ++r) step(K[r], n + r);
      }
      if (nn > 0) fold();
      // The axial nodes in node order: SQ receives the terms of one member's axial nodes, and the
      // member's sum is added to F where its last axial node has been taken: F += SQ cq after the
      // members' transverse sums, not (SQ cq + S1 c1) + S2 c2 inside them.
      {
        int ma = 0, mq = -1;   // the member of the node, and of the terms SQ holds
        auto flush = [&]() {
#pragma unroll
          for (int i = 0; i < 6; ++i) F[i] = add(F[i], scl(SQ, mbf[18 * mq + RH_MF_CQ0 + i]));
          SQ = mk(0, 0);
        };
        for (int k0 = 0; k0 < nn; k0 += kAxC) {
          if (ax_node(k0) < 0) break;   // uniform: the end of the list
#pragma unroll
          for (int r = 0; r < kAxC; ++r) {
            const int n = ax_node(k0 + r);
            if (n >= 0) {   // uniform
              while (n >= __builtin_amdgcn_readfirstlane(mstart[ma + 1])) ++ma;
              if (ma != mq) {
                if (mq >= 0) flush();
                mq = ma;
              }
              SQ = add(SQ, scl(KQ[r], al[6 * n]));
              load_axial(KQ[r], k0 + r + kAxC);
            }
          }
        }
        if (mq >= 0) flush();
      }
    }
    const double z = lz[bj];
#pragma unroll
    for (int c = 0; c < 6; ++c) F[c] = add(scl(fe[c], z), scl(F[c], z));   // F_lin + F_drag
    if (has_fx) {
      cd fx[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) fx[c] = bld(bFx, vj, c * nw16);
#pragma unroll
      for (int c = 0; c < 6; ++c) F[c] = add(F[c], mk(okj ? fx[c].r : 0.0, okj ? fx[c].i : 0.0));
    }
  };
  // The same for both bins of this thread in one sweep (JC): F[j] of bin tid + LT j.  Per bin the
  // operations and their order are excite's, so the bits are; what is shared is everything that does
  // not depend on the bin: the member test, fold()'s and flush()'s factor reads, the node's `al` row,
  // the scalar row offsets.  The ring's kRingC slots hold one (node, bin) each, in the order they are
  // consumed (node n bin 0, node n bin 1, node n + 1 bin 0, ...): each is waited for by itself, so
  // every wait still leaves the other kRingC - 1 slots' rows outstanding, and each is refilled with
  // the same bin of node n + kRingCJ once it is consumed.
  auto excite2 = [&](cd (&F)[2][6]) {
    unsigned vj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) vj[j] = voff(tid + LT * j);
    // (unit inertial excitation of the two bins: requested behind the node loop, in flight during
    // the axial loop -- 48 VGPRs that the node loop, with both bins' sums and F, has no room for)
    cd fe[2][6];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < 6; ++c) F[j][c] = mk(0, 0);
    {
      cd SQ[2], S1[2], S2[2], T1[2], T2[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) SQ[j] = S1[j] = S2[j] = T1[j] = T2[j] = mk(0, 0);
      auto load1 = [&](cd (&K)[2], int n, int j) {
        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;
#pragma unroll
        for (int p = 0; p < 2; ++p) K[p] = bld(bK, vj[j], so + (unsigned)(p + 1) * nw16);
      };
      auto load_axial = [&](cd (&Kq)[2], int k) {   // row 0 of the k-th axial node (none past the list)
        const int n = ax_node(k);
        if (n >= 0) {   // uniform
#pragma unroll
          for (int j = 0; j < 2; ++j) Kq[j] = bld(bK, vj[j], (unsigned)n * 3u * nw16);
        } else {
          Kq[0] = Kq[1] = mk(0.0, 0.0);
        }
      };
      int m = 0, mnext = nn > 0 ? mstart[1] : 0;
      auto fold = [&]() {   // close member m: F += sum of its nodes, the factors read once for both bins
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const double c1 = mbf[18 * m + RH_MF_C10 + i], c2 = mbf[18 * m + RH_MF_C20 + i];
#pragma unroll
          for (int j = 0; j < 2; ++j) F[j][i] = add(F[j][i], add(scl(S1[j], c1), scl(S2[j], c2)));
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double p1 = mbf[18 * m + RH_MF_C10 + i], p2 = mbf[18 * m + RH_MF_C20 + i];
#pragma unroll
          for (int j = 0; j < 2; ++j) F[j][3 + i] = add(F[j][3 + i], sub(scl(T1[j], p2), scl(T2[j], p1)));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) S1[j] = S2[j] = T1[j] = T2[j] = mk(0, 0);
      };
      // (the axial rows first, then the ring in slot order, each slot scheduled by itself: as excite)
      cd KQ[kAxC][2];
#pragma unroll
      for (int r = 0; r < kAxC; ++r) load_axial(KQ[r], nn > 0 ? r : nn);
      __builtin_amdgcn_sched_barrier(0);
      cd K[kRingCJ][2][2];   // [node slot][bin][row]
#pragma unroll
      for (int r = 0; r < kRingCJ; ++r) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          load1(K[r][j], r, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      double A1 = al[1], A2 = al[2], A3 = al[3], A4 = al[4];
      auto step = [&](cd (&K)[2][2], int n) {
        while (n == mnext) {   // uniform: member m ended before node n
          fold();
          ++m;
          mnext = mstart[m + 1];
        }
        const double a1 = A1, a2 = A2, a3 = A3, a4 = A4;
        {
          const double* A = al + 6 * (n + 1 < nn ? n + 1 : nn);
          A1 = A[1]; A2 = A[2]; A3 = A[3]; A4 = A[4];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          S1[j] = add(S1[j], scl(K[j][0], a1));
          S2[j] = add(S2[j], scl(K[j][1], a2));
          T1[j] = add(T1[j], scl(K[j][0], a3));
          T2[j] = add(T2[j], scl(K[j][1], a4));
          __builtin_amdgcn_sched_barrier(0);   // consumed before the refill is issued
          load1(K[j], n + kRingCJ, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
#pragma unroll 1
      for (int n = 0; n < nn; n += kRingCJ) {   // whole rounds: the last one ends in ghost nodes
#pragma unroll
        for (int r = 0; r < kRingCJ; ++r) step(K[r], n + r);
      }
      if (nn > 0) fold();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < 6; ++c) fe[j][c] = bld(bFe, vj[j], c * nw16);
      {
        int ma = 0, mq = -1;   // the member of the node, and of the terms SQ holds
        auto flush = [&]() {
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const double cq = mbf[18 * mq + RH_MF_CQ0 + i];
#pragma unroll
            for (int j = 0; j < 2; ++j) F[j][i] = add(F[j][i], scl(SQ[j], cq));
          }
          SQ[0] = SQ[1] = mk(0, 0);
        };
        for (int k0 = 0; k0 < nn; k0 += kAxC) {
          if (ax_node(k0) < 0) break;   // uniform: the end of the list
#pragma unroll
          for (int r = 0; r < kAxC; ++r) {
            const int n = ax_node(k0 + r);
            if (n >= 0) {   // uniform
              while (n >= __builtin_amdgcn_readfirstlane(mstart[ma + 1])) ++ma;
              if (ma != mq) {
                if (mq >= 0) flush();
                mq = ma;
              }
              const double aq = al[6 * n];
#pragma unroll
              for (int j = 0; j < 2; ++j) SQ[j] = add(SQ[j], scl(KQ[r][j], aq));
              load_axial(KQ[r], k0 + r + kAxC);
            }
          }
        }
        if (mq >= 0) flush();
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double z = lz[tid + LT * j];
#pragma unroll
      for (int c = 0; c < 6; ++c) F[j][c] = add(scl(fe[j][c], z), scl(F[j][c], z));   // F_lin + F_drag
    }
    if (has_fx) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool okj = tid + LT * j < nw;
        cd fx[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) fx[c] = bld(bFx, vj[j], c * nw16);
#pragma unroll
        for (int c = 0; c < 6; ++c) F[j][c] = add(F[j][c], mk(okj ? fx[c].r : 0.0, okj ? fx[c].i : 0.0));
      }
    }
  };

  const double hdw = 0.5 / d.dw;   // psd = |x|^2 hdw and rao = x (1 / zeta): multiplies, not 36 divisions per thread
  // What the removed two-pass launch left in the device code: its default stop
  // iteration was the constant 1 << 30, which the compiler cannot prove >= nloop, so the shipped
  // kernels have always carried this cap and the park-and-stop block of the epilogue below.  No
  // call reaches them (nIter < 2^30), but without them every k_solve_lds instantiation gets
  // another register allocation (254 instead of 255 VGPRs in <2, 512>, which tests/test_isa_joint_c.py
  // pins): they go in a change with its own timing.
  constexpr int kIterCap = 1 << 30;
  const int itend = kIterCap >= nloop ? nloop : kIterCap;
  for (int it = it0; it < itend; ++it) {
    PROF_T(ta0);
    PROF_ADD(7, 1);
    // ---------------- A: per-node sums of squared relative-velocity components ----------
    // Member-factored (rh_member_field): per (member, bin)
    //   Bq = iw cq.Xi, B1 = iw c1.Xi, B2 = iw c2.Xi, E1 = iw p2.th, E2 = -iw p1.th
    // and per node s_q = z Kq - Bq, s_1 = z K1 - (B1 + t E1), s_2 = z K2 - (B2 + t E2)
    // (raft/raft_fowt.py:1205-1211).
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {   // passes of NWP bins (NP == 1: the whole grid)
      const int pb = tid + NWP * p;  // this thread's first bin of the pass
      unsigned vb[NB];
      double bz[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        vb[j] = voff(pb + LT * j);
        bz[j] = lz[pb + LT * j];
      }
      cd XR[GX ? NB : 1][6];         // GX: the pass's XiLast, loaded before the node loop
      if constexpr (GX) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int b = pb + LT * j, bc = b < nw ? b : nw - 1;
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const cd v = ld(XL + c * nw + bc);
            XR[j][c] = b < nw ? v : mk(0.0, 0.0);
          }
        }
      }
      // (defined here, not just before their first use: left undefined, the register allocator
      // may keep the previous iteration's values live, and spill them, across phase C)
      cd B1[NB], B2[NB], E1[NB], E2[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) B1[j] = B2[j] = E1[j] = E2[j] = mk(0.0, 0.0);
      auto bin_xi = [&](int j, cd (&X)[6]) {   // XiLast of bin j of this thread
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          if constexpr (GX) X[c] = XR[j][c];
          else X[c] = xl[c * NWP + pb + LT * j];
        }
      };
      auto member_terms = [&](int m) {   // the transverse terms of member m
        double c1[6], c2[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          c1[i] = mbf[18 * m + RH_MF_C10 + i];
          c2[i] = mbf[18 * m + RH_MF_C20 + i];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          cd X[6];
          bin_xi(j, X);
          cd A1 = mk(0, 0), A2 = mk(0, 0);
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            A1 = add(A1, scl(X[c], c1[c]));
            A2 = add(A2, scl(X[c], c2[c]));
          }
          const cd D1 = add(add(scl(X[3], c2[0]), scl(X[4], c2[1])), scl(X[5], c2[2]));   // p2 . th
          const cd D2 = add(add(scl(X[3], c1[0]), scl(X[4], c1[1])), scl(X[5], c1[2]));   // p1 . th
          const double w = lw[pb + LT * j];
          B1[j] = iw(w, A1);
          B2[j] = iw(w, A2);
          E1[j] = iw(w, D1);
          E2[j] = iw(-w, D2);
        }
      };
      auto axial_term = [&](int m, cd (&Bq)[NB]) {   // Bq of member m (axial nodes only)
        double cq[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) cq[i] = mbf[18 * m + RH_MF_CQ0 + i];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          cd X[6];
          bin_xi(j, X);
          cd Aq = mk(0, 0);
#pragma unroll
          for (int c = 0; c < 6; ++c) Aq = add(Aq, scl(X[c], cq[c]));
          Bq[j] = iw(lw[pb + LT * j], Aq);
        }
      };
      // The streaming loop over all nodes carries the two transverse rows only; the axial rows
      // of the few nodes that need them (ax_node) are summed in a short loop of their own
      // after it (nothing couples s_q to s_1 and s_2).
      auto load_node = [&](cd (&K)[2][NB], int n) {
        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int p = 0; p < 2; ++p) K[p][j] = bld(bK, vb[j], so + (unsigned)(p + 1) * nw16);
      };
      auto load_axial = [&](cd (&K)[NB], int k) {   // row 0 of the k-th axial node (none past the list)
        const int n = ax_node(k);
        if (n >= 0) {   // uniform
          const unsigned so = (unsigned)n * 3u * nw16;
#pragma unroll
          for (int j = 0; j < NB; ++j) K[j] = bld(bK, vb[j], so);
        } else {
#pragma unroll
          for (int j = 0; j < NB; ++j) K[j] = mk(0.0, 0.0);
        }
      };
      // this lane's partial sums over its bins of |s_1|^2, |s_2|^2 for one node
      auto node_sums = [&](const cd (&K)[2][NB], double t, double& s1, double& s2) {
        s1 = s2 = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const double z = bz[j];
          const cd sp1 = sub(scl(K[0][j], z), add(B1[j], scl(E1[j], t)));
          const cd sp2 = sub(scl(K[1][j], z), add(B2[j], scl(E2[j], t)));
          s1 += abs2(sp1);
          s2 += abs2(sp2);
        }
      };
      // Ring depth 4 (one pass): the sums of a ring round's four nodes reduced together (tbfly8) and the
      // axial sums of four nodes per tbfly4; depth 3 (two-pass GX): tbfly3 per node, and per three axial
      // nodes.  (Two nodes per butterfly measured slower than four)
      static_assert(kRingA == 4 || kRingA == 3, "phase A reduces a round of 4 nodes (tbfly8) or single nodes at depth 3");
      constexpr bool kQuad = kRingA == 4;
      constexpr int kAx = kQuad ? 4 : 3;   // axial nodes per butterfly
      // The first kAx axial rows are requested before the ring's, so they arrive behind the
      // transverse loop; a design with more axial nodes waits once per further kAx of them.
      cd KQ[kAx][NB];
#pragma unroll
      for (int r = 0; r < kAx; ++r) load_axial(KQ[r], nn > 0 ? r : nn);
      // The ring slot of node n is refilled with node n + kRingA.
      cd K[kRingA][2][NB];
#pragma unroll
      for (int r = 0; r < kRingA; ++r) {   // in ring order (see phase C)
        load_node(K[r], r);
        __builtin_amdgcn_sched_barrier(0);
      }
      int m = -1, mnext = 0;
      [[maybe_unused]] double u8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (kQuad) the sums of a round's nodes
      // (kQuad) the butterfly's lane flags: formed here, live through the node loops only
      // (lane_here is not hoisted out of the iteration loop)
      const Bfly4 bl = bfly4_lane(kQuad ? lane_here() : 0);
      // Whole ring rounds: the last one ends in ghost nodes (the last node's rows again), whose sums
      // are reduced like any other's and written nowhere.  node n's t is read a node ahead.
      double tn = nt[0];
#pragma unroll 1
      for (int n = 0; n < nn; n += kRingA) {
#pragma unroll
        for (int r = 0; r < kRingA; ++r) {
          const int nr = n + r;
          if (nr == mnext) {   // uniform: entering member m+1 (members are node-contiguous)
            do { ++m; mnext = mstart[m + 1]; } while (mnext == nr);
            member_terms(m);
          }
          double s1, s2;
          node_sums(K[r], tn, s1, s2);
          // The slot's rows are consumed here, before its refill is issued.  Without the member
          // boundaries' merge points between them nothing else holds the sums in place: they are used
          // only by the round's butterfly, the compiler sinks them down to it, every slot's old rows
          // stay live beside their refills, and the ring spills (the opaque statement pins them).
          asm volatile("" : "+v"(s1), "+v"(s2));
          tn = nt[nr + 1 < nn ? nr + 1 : nn];
          load_node(K[r], nr + kRingA);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (kQuad) {
            u8[2 * r] = s1;
            u8[2 * r + 1] = s2;
            if (r == kRingA - 1) {   // (folded by the unrolling)
              const double tot = tbfly8(u8, bl);
              if (bl.vi8 >= 0 && n + (bl.vi8 >> 1) < nn) {
                double& rr = red[((n + (bl.vi8 >> 1)) * 3 + 1 + (bl.vi8 & 1)) * LW + wv_s];
                rr = (GX && p > 0) ? rr + tot : tot;   // passes add in pass order
              }
            }
          } else {
            const double tot = tbfly3(s1, s2, 0.0);
            const int vi = tbfly3_index(lane_here());
            if (vi >= 0 && vi < 2 && nr < nn) {   // lanes 0, 16
              double& rr = red[(nr * 3 + 1 + vi) * LW + wv_s];
              rr = (GX && p > 0) ? rr + tot : tot;   // passes add in pass order
            }
          }
        }
      }
      // the axial nodes, kAx per butterfly, each with the Bq of its member
      int ma = 0;
      for (int k0 = 0; k0 < nn; k0 += kAx) {
        if (ax_node(k0) < 0) break;   // uniform: the end of the list
        double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < kAx; ++r) {
          const int n = ax_node(k0 + r);
          if (n >= 0) {   // uniform
            while (n >= __builtin_amdgcn_readfirstlane(mstart[ma + 1])) ++ma;
            cd Bq[NB];
            axial_term(ma, Bq);
            double s0 = 0;
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              const cd sq = sub(scl(KQ[r][j], bz[j]), Bq[j]);
              s0 += abs2(sq);
            }
            q[r] = s0;
            load_axial(KQ[r], k0 + r + kAx);
          }
        }
        int vi;
        double tot;
        if constexpr (kQuad) {
          tot = tbfly4(q[0], q[1], q[2], q[3]);
          vi = bl.vi;
        } else {
          tot = tbfly3(q[0], q[1], q[2]);
          vi = tbfly3_index(lane_here());
        }
        if (vi >= 0 && k0 + vi < nn) {
          const int n = ax[12 * (k0 + vi) + 11];
          if (n >= 0) {
            double& rr = red[n * 3 * LW + wv_s];
            rr = (GX && p > 0) ? rr + tot : tot;   // passes add in pass order
          }
        }
      }
    }
    __syncthreads();
    if constexpr (kOv) {
      // the deferred vote of iteration it - 1 (every wave finished its phase C before this
      // barrier; they came here because some test of it - 1 failed, so it did not converge)
      if (it > it0) {
        const int fl = sflag[(it - 1) & 1];
        if (a.o.margin && tid == 0) margin = closer_call(margin, wave_maxes(mred) - tol);
        if (fl & 6) {
          status = (fl & 2) ? RH_CASE_NAN : RH_CASE_SINGULAR;
          iters = it;
          break;
        }
      }
    }
    PROF_T(ta1);
    PROF_ADD(1, ta1 - ta0);
    // ---------------- B: node drag matrices and B_drag ----------------------------------
    // (the batched form indexes with the thread's number formed anew, here and in the node sum below: the
    // LDS addresses that follow from a hoisted copy are computed once before the iteration loop and stay
    // live across the solve, where two more of them cost the kernel a 256th VGPR and the one-bin kernels
    // four more spilled ones)
    const int tid_b = kBatchS ? wv_s * 64 + lane_here() : tid;
    for (int n = tid_b; n < nn; n += LT) {
      // the node's fields XX .. CIRC and T, all loads issued before any use (left to the
      // scheduler, each load waited on before the next was issued: eight serial L2 round trips)
      double fv[RH_NF_CIRC - RH_NF_XX + 2];
#pragma unroll
      for (int f = RH_NF_XX; f <= RH_NF_CIRC; ++f) fv[f - RH_NF_XX] = node[(size_t)f * nn + n];
      fv[RH_NF_CIRC - RH_NF_XX + 1] = node[(size_t)RH_NF_T * nn + n];
      __builtin_amdgcn_sched_barrier(0);
      auto F = [&](int f) { return f == RH_NF_T ? fv[RH_NF_CIRC - RH_NF_XX + 1] : fv[f - RH_NF_XX]; };
      double r3[3];
      if constexpr (kBatchS) {
        // the 3 LW wave partials, every read issued before the first add (left to the scheduler, each
        // pair of partials was read, waited for and added in turn: 12 serial LDS round trips at LW = 8);
        // summed in wave order as before, while the field loads above are still in flight
        double pr[3][LW];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int w = 0; w < LW; ++w) pr[c][w] = red[(size_t)(n * 3 + c) * LW + w];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double s = 0;
#pragma unroll
          for (int w = 0; w < LW; ++w) s += pr[c][w];
          r3[c] = s;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double* R = red + (size_t)(n * 3 + c) * LW;
          double s = 0;
#pragma unroll
          for (int w = 0; w < LW; ++w) s += R[w];
          r3[c] = s;
        }
      }
      // a node that does not need its axial sum has none (phase A wrote no partials for it): an
      // exact 0, so vq = 0 and Bq = Be = +0, the zeros that its zero coefficients give anyway
      if (!(ax[12 * n + 10] & 1)) r3[0] = 0.0;
      // sum|vrel_q|^2 = sum|s_q|^2 |q|^2 ; circular: |vrel_p|^2 = |s_1|^2|p1|^2 + |s_2|^2|p2|^2
      auto n2 = [&](int f) { const double a = F(f), b = F(f + 1), c = F(f + 2); return a * a + b * b + c * c; };
      const double qq = n2(RH_NF_QX), pp1 = n2(RH_NF_P1X), pp2 = n2(RH_NF_P2X);
      const bool circ = F(RH_NF_CIRC) != 0.0;
      const double sums[3] = {r3[0] * qq, circ ? r3[1] * pp1 + r3[2] * pp2 : r3[1] * pp1, r3[2] * pp2};
      double B4[4];
      // The node's Bmat stays in registers for the 36 translate entries below.  Read back from the LDS
      // row, every entry's operands were loaded anew behind the stores of the entries before it and waited
      // for with a full drain (the stores to bdn, a double* into the same array, may alias bm for all the
      // compiler knows): 73 drains per node.  The row is still written, for the epilogue's Bmat output.
      double Bn[9];
      if constexpr (kBatchS) {
        node_bmat_f(F, rho, sums, Bn, B4);
#pragma unroll
        for (int k = 0; k < 9; ++k) bm[9 * n + k] = Bn[k];
      } else {
        node_bmat_f(F, rho, sums, bm + 9 * n, B4);
      }
      const double t = F(RH_NF_T);
      double* A = al + 6 * n;
      A[0] = B4[0] + B4[3];     // axial: side + end   (qMat terms of Bmat, raft/raft_fowt.py:1228-1248)
      A[1] = B4[1];
      A[2] = B4[2];
      A[3] = t * B4[1];
      A[4] = t * B4[2];
      if (!SER) {
        // this node's translateMatrix3to6DOF (raft/helpers.py:455-478), summed below in node order
        const double rx = F(RH_NF_XX), ry = F(RH_NF_XY), rz = F(RH_NF_XZ);
#pragma unroll
        for (int e = 0; e < 36; ++e)
          bdn[e * nn + n] = kBatchS ? t3to6_fma(Bn, rx, ry, rz, e / 6, e % 6) : t3to6(bm + 9 * n, rx, ry, rz, e / 6, e % 6);
      }
    }
    __syncthreads();
    if (SER) {
      // B_drag without the per-node image: the 27 distinct entries of translateMatrix3to6DOF (9 of
      // Bm, 9 of Bm H, 9 of H Bm H^T; the lower-left block is the transpose of the upper-right
      // one) of cn nodes at a time go to the node-sum buffer (free after the Bmat loop above), one
      // thread per node computing them with t3to6's expressions; lane e < 27 then adds entry e of
      // those nodes to its running sum in node order (the same bits as the image path).
      const int cn = (nn * 3 * LW) / 27 > 0 ? (nn * 3 * LW) / 27 : 1;
      double se = 0.0;
      for (int n0 = 0; n0 < nn; n0 += cn) {
        const int cnt = nn - n0 < cn ? nn - n0 : cn;
        for (int nl = tid; nl < cnt; nl += LT) {   // one node per thread: its 27 entries share the loads
          const int n = n0 + nl;
          const double rx = nf(node, nn, RH_NF_XX, n), ry = nf(node, nn, RH_NF_XY, n), rz = nf(node, nn, RH_NF_XZ, n);
          double Bn[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) Bn[k] = bm[9 * n + k];
#pragma unroll
          for (int e = 0; e < 27; ++e) red[27 * nl + e] = t3to6_block(Bn, rx, ry, rz, e / 9, (e % 9) / 3, e % 3);
        }
        __syncthreads();
        if (tid < 27)
          for (int k = 0; k < cnt; ++k) se += red[27 * k + tid];
        __syncthreads();
      }
      if (tid < 27) {
        const int blk = tid / 9, r = (tid % 9) / 3, c = tid % 3;
        if (blk == 0) bd[6 * r + c] = se;
        else if (blk == 1) bd[6 * r + 3 + c] = bd[6 * (3 + c) + r] = se;
        else bd[6 * (3 + r) + 3 + c] = se;
      }
      __syncthreads();
      if (tid < 36) bsum[tid] = mbc[36 + tid] + bd[tid];
    } else if (tid < 36) {
      double s = 0;
      // (tid < 36: wave 0, lane = tid.  The lane formed anew: the batched form reads from two addresses
      // that follow from tid, which are computed once before the iteration loop and stay live across the
      // solve; with tid itself the kernel took one VGPR more.)
      const double* P = bdn + (kBatchS ? lane_here() : tid) * nn;
      if constexpr (kBatchS) {
        // kSumB nodes' entries read before their adds, the adds strictly in node order (the plain loop
        // ran as one LDS round trip per two nodes).  The last batch reads kSumB - 1 words from its first
        // node on and adds those of the nodes there are: the words past the row belong to the next entry's
        // row or, behind the last row, to nt and lw (at least 128 doubles), so they are inside the block.
        int n = 0;
        for (; n + kSumB <= nn; n += kSumB) {
          double p[kSumB];
#pragma unroll
          for (int k = 0; k < kSumB; ++k) p[k] = P[n + k];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < kSumB; ++k) s += p[k];
        }
        if (n < nn) {
          double p[kSumB - 1];
#pragma unroll
          for (int k = 0; k < kSumB - 1; ++k) p[k] = P[n + k];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < kSumB - 1; ++k)
            if (n + k < nn) s += p[k];
        }
      } else {
        for (int n = 0; n < nn; ++n) s += P[n];
      }
      bd[tid] = s;
      bsum[tid] = mbc[36 + tid] + s;   // the B_lin + B_drag of every bin's Z (same sum as before)
    }
    __syncthreads();
    PROF_T(ta2);
    PROF_ADD(2, ta2 - ta0 - (ta1 - ta0));
#ifdef RH_PROF
    unsigned long long tc_exc = 0, tc_sol = 0, tc_z = 0, tc_lu = 0;
#endif
    // ---------------- C: excitation, Z(w), LU solve, convergence flags ------------------
    bool my_ok = true, my_nan = false, my_sing = false;
    double tN = 0.0, tD = 1.0;   // the lane's largest tolCheck so far as tt^2 = tN / tD
    // the last allowed iteration stores every entry of the unrelaxed iterate (uniform)
    const bool last_it = __builtin_amdgcn_readfirstlane(it + 1 == nloop ? 1 : 0) != 0;
    // The outputs of the final iteration (Xi, F_wave) are stored by every iteration that may be
    // the final one: the last allowed, or one whose tests have all passed so far.  A wave that
    // sees a failed test (any lane, this bin or an earlier one) marks the iteration in LDS
    // (sflag[2]); the other waves read the mark at their next store (a stale read only stores
    // more).  (uniform)
    auto may_be_final = [&]() -> bool {
      if (last_it) return true;
      if (__builtin_amdgcn_ballot_w64(!my_ok)) {
        if (lane == 0) __hip_atomic_store(&sflag[2], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return false;
      }
      return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&sflag[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != it + 1;
    };
    if constexpr (kStatsC)
      if (lane < 6) sred[wv * 6 + lane] = 0.0;   // this wave's RMS sums: only the final iteration's are kept
    if constexpr (kOv) {
      // the words of iteration it + 1: their last readers (iteration it - 1's vote) are done
      if (tid == 0) {
        sflag[(it + 1) & 1] = 0;
        sflag[3 + ((it + 1) & 1)] = 0;
      }
    }
#pragma unroll 1
    for (int j = 0; j < NBT; ++j) {
      // per-bin scalars picked without dynamic register indexing (the loop is not unrolled,
      // so only one bin's LU is ever live)
      const int bj = tid + LT * j;
      const bool okj = bj < nw;
      PROF_T(tc0);
      cd F[6];
      if constexpr (JC) {
        // One sweep at bin 0 forms both bins' F.  Bin 1's is not kept in registers across bin 0's
        // LU (24 VGPRs beside Z and F: the round-2 joint sweep spilled 113 for it): its six entries
        // are parked in global memory, in rows only this thread touches, and read back here, where
        // the loads' latency runs under the Z build from LDS; no streaming loop is near either end.
        // The block is the case's Xi rows of bin 1, else its Xi_last rows (the one-pass kernels
        // leave them unused), else its F_wave rows (the host launches k_solve_lds_split when a call
        // has none of the three).  What a caller reads does not change: every iteration that may be
        // the final one stores bin 1's Xi (and F_wave) below, after this read-back, so the final
        // iteration overwrites the parked values with what the one-sweep-per-bin kernel stores; an
        // iteration that cannot be final is followed by one that does; and a case that fails (NaN,
        // singular) has its outputs overwritten with NaN in the epilogue.
        rh_c128* PK = (Xo ? Xo : a.o.Xi_last ? a.o.Xi_last + c6 : a.o.F_wave + c6) + bj;
        if (j == 0) {   // uniform
          cd F2[2][6];
          excite2(F2);
#pragma unroll
          for (int c = 0; c < 6; ++c) F[c] = F2[0][c];
          if (bj + LT < nw) {
#pragma unroll
            for (int c = 0; c < 6; ++c) st(PK + LT + c * nw, F2[1][c]);
          }
        } else {
#pragma unroll
          for (int c = 0; c < 6; ++c) F[c] = mk(0.0, 0.0);   // pad lanes: zeta = 0 gave F = 0
          if (okj) {
#pragma unroll
            for (int c = 0; c < 6; ++c) F[c] = ld(PK + c * nw);
          }
        }
      } else {
        excite(bj, F);
      }
      // F_wave: the excitation of the final iteration, which every iteration's overwrites (F is
      // live for the LU anyway), skipped once the iteration is known not to be final (below)
      if (a.o.F_wave && may_be_final()) {
        if (okj) {
#pragma unroll
          for (int c = 0; c < 6; ++c) st_nt(a.o.F_wave + c6 + c * nw + bj, F[c]);
        }
      }
      PROF_T(tc1);
#ifdef RH_PROF
      tc_exc += tc1 - tc0;
#endif
      // No lane branch around the solve (a per-lane `continue` here let the compiler's spills
      // run under a partial EXEC mask in the general kernel): only a wave whose
      // every lane is past the grid skips it (uniform); pad lanes of the last wave solve the
      // clamped last bin with a zero right-hand side (zeta = 0, x = 0 exactly) and store nothing.
      if (!__builtin_amdgcn_ballot_w64(okj)) continue;
      const int b = bj;
      const double w = lw[b];
      cd Z[6][6];
      {
        // index the LDS image with a zero the compiler cannot see through, so that its 144
        // loop-invariant reads stay here instead of being hoisted into VGPRs for the solve
        const int zo = opaque_zero();
        const double* zm = mbc + zo;
        const double* zb = bd + zo;
        const double* zs = bsum + zo;
        const double w2 = -(w * w);
        if (d.mb_per_bin) {
          const int bc = okj ? b : nw - 1;
          const double* M = d.M + (size_t)bc * 36;
          const double* B = d.B + (size_t)bc * 36;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) Z[r][c] = mk(w2 * M[6 * r + c] + zm[72 + 6 * r + c], w * (B[6 * r + c] + zb[6 * r + c]));
            __builtin_amdgcn_sched_barrier(0);   // one row of reads in flight at a time
          }
        } else {
#pragma unroll
          for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c)
              Z[r][c] = mk(w2 * zm[6 * r + c] + zm[72 + 6 * r + c], w * zs[6 * r + c]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
#ifdef RH_PROF
      const unsigned long long tcz = clock64();
      tc_z += tcz - tc1;
#endif
      const bool ok_lu = lu_solve<6>(Z, F);
      my_sing |= okj && !ok_lu;
#ifdef RH_PROF
      tc_lu += clock64() - tcz;
#endif
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const cd x = F[c];
        cd xlast;
        if constexpr (GX) {
          const cd v = ld(XL + c * nw + (okj ? b : nw - 1));
          xlast = okj ? v : mk(0.0, 0.0);
        } else {
          xlast = xl[c * NWP + b];
        }
        my_nan |= okj && ((x.r != x.r) || (x.i != x.i));
        // tolCheck = |Xi - XiLast| / (|Xi| + tol) < tol  (raft/raft_model.py:961-962)
        // (magnitudes as sqrt(re^2 + im^2): within an ulp of np.abs's hypot, far cheaper)
        // tt < tol as |Xi - XiLast|^2 < (tol (|Xi| + tol))^2: one square root, no division per
        // entry; the lane keeps its largest tt^2 as a fraction (compared by cross products) and
        // forms tt itself only for the convergence margin, once per iteration
        const double n2 = abs2(sub(x, xlast)), den = sqrt(abs2(x)) + tol, d2 = den * den;
        const double td = tol * den;
        my_ok = my_ok && (!okj || n2 < td * td);
        const bool gt = okj && n2 * tD > tN * d2;
        tN = gt ? n2 : tN;
        tD = gt ? d2 : tD;
        if (okj && XP) st(XP + c * nw + b, xlast);
        // XiLast = 0.2 XiLast + 0.8 Xi  (:991), only consumed if not converged (pads: 0)
        const cd xr = add(scl(xlast, 0.2), scl(x, 0.8));
        if constexpr (GX) {
          if (okj) st(XL + c * nw + b, xr);
        } else {
          xl[c * NWP + b] = xr;
        }
      }
      // The unrelaxed iterate leaves the kernel only as the output of the case's final
      // iteration: the one whose test every (bin, DOF) passed, or the last allowed one
      // (raft/raft_model.py:996-1000).  So the bin's six entries are stored only while this
      // iteration may still be that one (may_be_final, with this bin's tests counted);
      // streamed: the final iteration's stores are the ones kept.  (Xi may be NULL with NP == 1.)
      if ((GX || Xo) && may_be_final()) {
        if constexpr (kStatsC) {
          // PSD, RAO and the RMS sums from x in registers (the epilogue's arithmetic,
          // k_motion_stats with one row): the final iteration's values are the ones kept, and
          // nothing is read back
          const double z = lz[b];
          const double rz = fabs(z) > 1e-6 ? 1.0 / z : 0.0;
          double m2v[6];
#pragma unroll
          for (int c = 0; c < 6; ++c) m2v[c] = okj ? abs2_re(c >= 3 ? scl(F[c], kRad2Deg) : F[c]) : 0.0;
          if (okj) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
              st_nt(Xo + c * nw + b, F[c]);
              if (a.o.psd) __builtin_nontemporal_store(m2v[c] * hdw, a.o.psd + ((size_t)ic * 6 + c) * nw + b);
              if (a.o.rao) st_nt(a.o.rao + ((size_t)ic * 6 + c) * nw + b, scl(F[c], rz));
            }
          }
          if (a.o.std) {   // the bin's six sums over the wave by two transposing butterflies
            const double t0 = tbfly3(m2v[0], m2v[1], m2v[2]), t1 = tbfly3(m2v[3], m2v[4], m2v[5]);
            const int k = tbfly3_index(lane_here());
            if (k >= 0) {   // lanes 0, 16, 32
              sred[wv * 6 + k] += t0;
              sred[wv * 6 + 3 + k] += t1;
            }
          }
        } else if (okj) {
#pragma unroll
          for (int c = 0; c < 6; ++c) st_nt(Xo + c * nw + b, F[c]);
        }
      }
#ifdef RH_PROF
      tc_sol += clock64() - tc1;
#endif
    }
    PROF_ADD(3, tc_exc);
    PROF_ADD(4, tc_sol);
    PROF_ADD(8, tc_z);
    PROF_ADD(9, tc_lu);
    PROF_T(ta3);
    if (a.o.margin) {
      const double my_tmax = sqrt(tN) / sqrt(tD);
      const double mw = wave_max(my_tmax);
      if (lane == 0) mred[wv] = mw;
    }
    if constexpr (kOv) {
      // No barrier here.  Each wave ORs its flag bits (1 = a bin not converged, 2 = NaN,
      // 4 = singular) into this iteration's word and counts itself done (release: the bits, the
      // mark and mred first).  A wave that knows the loop goes on (one of its own tests failed,
      // or another wave's mark) starts the next phase A at once, overlapping the waves still in
      // phase C: phase A reads only the XiLast entries this very thread wrote, and writes only
      // the node partials, which phase B consumed before this iteration's phase C.  The vote is
      // then read after the next phase-A barrier (above).  Otherwise the wave waits for every
      // wave to be done or for a mark, whichever comes first; with all done and no mark the
      // iteration is the final one, the same verdict for every wave (a mark is written before
      // its wave's done count).  The last allowed iteration always waits for all.
      const bool last = it + 1 == nloop;
      const unsigned long long bn = __builtin_amdgcn_ballot_w64(!my_ok), bx = __builtin_amdgcn_ballot_w64(my_nan),
                               bs = __builtin_amdgcn_ballot_w64(my_sing);
      const int bits = (bn ? 1 : 0) | (bx ? 2 : 0) | (bs ? 4 : 0);
      if (lane == 0) {
        if (bits) __hip_atomic_fetch_or(&sflag[it & 1], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (bn) __hip_atomic_store(&sflag[2], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&sflag[3 + (it & 1)], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      bool go_on = !last && bn != 0;
      if (!go_on) {
#pragma unroll 1
        while (true) {
          const int dn = __builtin_amdgcn_readfirstlane(
              __hip_atomic_load(&sflag[3 + (it & 1)], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
          const int mk = __builtin_amdgcn_readfirstlane(
              __hip_atomic_load(&sflag[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (!last && mk == it + 1) {
            go_on = true;
            break;
          }
          if (dn == LW) break;
          __builtin_amdgcn_s_sleep(1);
        }
      }
      PROF_T(ta4);
      PROF_ADD(5, ta4 - ta3);
      if (go_on) continue;
      // the final iteration: every wave is done and no test failed (or it was the last allowed)
      const int fl = __builtin_amdgcn_readfirstlane(
          __hip_atomic_load(&sflag[it & 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (a.o.margin && tid == 0) margin = closer_call(margin, wave_maxes(mred) - tol);
      status = (fl & 2) ? RH_CASE_NAN : (fl & 4) ? RH_CASE_SINGULAR : (fl & 1) ? RH_CASE_NOT_CONVERGED : RH_CASE_CONVERGED;
      iters = it + 1;
      break;
    } else {
    // (three barrier votes; one barrier with an LDS flag word moved the launch not at all)
    const int all_ok = __syncthreads_and(my_ok ? 1 : 0);
    if (a.o.margin && tid == 0) {   // mred is rewritten only after the next phase-A barrier
      double mx = mred[0];
      for (int w = 1; w < LW; ++w) mx = fmax(mx, mred[w]);
      margin = closer_call(margin, mx - tol);
    }
    const int any_nan = __syncthreads_or(my_nan ? 1 : 0);
    const int any_sing = __syncthreads_or(my_sing ? 1 : 0);
    PROF_T(ta4);
    PROF_ADD(5, ta4 - ta3);
    if (any_nan) {
      status = RH_CASE_NAN;
      iters = it + 1;
      break;
    }
    if (any_sing) {
      status = RH_CASE_SINGULAR;
      iters = it + 1;
      break;
    }
    if (all_ok) {
      status = RH_CASE_CONVERGED;
      iters = it + 1;
      break;
    }
    }
  }

  if (status == RH_CASE_NOT_CONVERGED && itend < nloop) {   // unreachable: see kIterCap
#pragma unroll 1
    for (int j = 0; j < NB && !GX; ++j) {
      const int b = tid + LT * j;
      if (b >= nw) continue;
#pragma unroll 1
      for (int c = 0; c < 6; ++c) st(a.o.Xi_last + c6 + c * nw + b, xl[c * NWP + b]);
    }
    if (tid == 0) {
      a.o.status[ic] = 9;
      if (a.o.margin) a.o.margin[ic] = margin;
    }
    return;
  }

  // ---------------- outputs ------------------------------------------------------------
#ifdef RH_WGTIME
  if (tid == 0 && blockIdx.x < 8192) {
    rh_wgt[2 * blockIdx.x] = wgt0;
    rh_wgt[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  PROF_T(te0);
  if (tid == 0) {
    a.o.iters[ic] = iters;
    a.o.status[ic] = status;
    if (a.o.margin) a.o.margin[ic] = margin;
  }
  if (a.o.B_drag && tid < 36) a.o.B_drag[(size_t)ic * 36 + tid] = bd[tid];
  if (a.o.Bmat)
    for (int e = tid; e < nn * 9; e += LT) a.o.Bmat[(size_t)ic * a.bmat_nn * 9 + e] = bm[e];
  if (a.o.Z) {   // final impedance fowt.Z (raft/raft_model.py:1013) from the last B_drag, streamed
#pragma unroll 1
    for (int j = 0; j < NBT; ++j) {
      const int b = tid + LT * j;
      if (b >= nw) continue;
      const double w = lw[b], w2 = -(w * w);
      rh_c128* Zo = a.o.Z + ((size_t)ic * nw + b) * 36;
#pragma unroll 1
      for (int e = 0; e < 36; ++e) {
        const double M = d.mb_per_bin ? d.M[(size_t)b * 36 + e] : mbc[e];
        const double B = d.mb_per_bin ? d.B[(size_t)b * 36 + e] : mbc[36 + e];
        st(Zo + e, mk(w2 * M + mbc[72 + e], w * (B + bd[e])));
      }
    }
  }
  // A case that stopped on a NaN or a singular Z has no response (the reference raises there,
  // raft/raft_model.py:957): its Xi, F_wave, PSD, RAO and std are NaN, as in k_solve_cases.  (The
  // entries of its last iterate were stored only where they passed their test.)
  const bool failed = status == RH_CASE_NAN || status == RH_CASE_SINGULAR;   // uniform
  if (failed && a.o.F_wave) {   // nor an excitation: an array solve of it gives NaN, not stale memory
#pragma unroll 1
    for (int j = 0; j < NBT; ++j) {
      const int b = tid + LT * j;
      if (b >= nw) continue;
#pragma unroll
      for (int c = 0; c < 6; ++c) st(a.o.F_wave + ((size_t)ic * 6 + c) * nw + b, mk(NAN, NAN));
    }
  }
  // (kStatsC: phase C formed PSD / RAO / the RMS sums of a case that did not fail)
  double ss[6] = {0, 0, 0, 0, 0, 0};
  if (!kStatsC || failed) {
#pragma unroll
  for (int j = 0; j < NBT; ++j) {
    const int b = tid + LT * j;
    if (b >= nw || !Xo) continue;   // (psd, std and rao need Xi: checked by the caller)
    const double z = lz[b];
    const double rz = fabs(z) > 1e-6 ? 1.0 / z : 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      cd x;
      if (failed) {
        x = mk(NAN, NAN);
        st(Xo + c * nw + b, x);
      } else {
        x = ld(Xo + c * nw + b);
      }
      const cd xd = c >= 3 ? scl(x, kRad2Deg) : x;
      const double m2 = abs2(xd);
      ss[c] += m2;
      if (a.o.psd) a.o.psd[((size_t)ic * 6 + c) * nw + b] = m2 * hdw;
      if (a.o.rao) st(a.o.rao + ((size_t)ic * 6 + c) * nw + b, failed ? x : scl(x, rz));
    }
  }
  }
  if (a.o.std) {
    if (!kStatsC || failed) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double s = wave_sum(ss[c]);
        if (lane == 0) sred[wv * 6 + c] = s;
      }
    }
    __syncthreads();
    if (tid < 6) {
      double s = 0;
      for (int w = 0; w < LW; ++w) s += sred[w * 6 + tid];
      a.o.std[(size_t)ic * 6 + tid] = sqrt(0.5 * s);
    }
  }
  PROF_T(te1);
  PROF_ADD(6, te1 - te0);
  // The register count the ISA tests pin ("The pinned register counts"): the LU's per-row
  // exchange left the two-bin 512-thread kernel 243 VGPRs (238 in the one-sweep-per-bin build) where the
  // tests hold 255 and 256.  An empty statement that names the last register of the pinned count makes the
  // compiler report that count; it emits no instruction, nothing is live here, and any count from 129 to
  // 256 is two waves per SIMD.  Not at the top of the kernel: there it cost 2 and 3 spilled VGPRs.
  if constexpr (NB == 2 && LT == kLT && !SER && NP == 1) {
    if constexpr (kJointC) asm volatile("" ::: "v254");
    else asm volatile("" ::: "v255");
  }
}

}  // namespace rh
