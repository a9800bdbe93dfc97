// rh_pose.hip -- per-pose strip-node / member tables and batched current loads on the device: the
// kernels over the host/device math of rh_pose.h, and their two ABI calls (rh_pose_designs,
// rh_current_loads).  Included by rh_abi.hip after its `fail` / RH_HIP helpers.
//
// k_pose_designs: one workgroup of 256 per pose.
//   A. one thread per member: its frame at the pose (rA, rB, q, p1, p2 and l) into LDS, and its
//      index into the LDS node -> member map;
//   B. counting sweep: nodes in passes of 256, one 64-node chunk per wave and pass; the chunk's
//      wet nodes (r_z < 0) as one ballot mask in LDS;
//   C. one thread: the chunks' exclusive offsets, nn, then the kept members (those with a wet
//      node), their slots, mstart and nm.  The rank of node j among the wet ones is
//      off[j / 64] + popcount(mask[j / 64] below bit j % 64);
//   D. writing sweep: every wet node's 36 fields at stride nn (known only now), the kept members'
//      21 fields at stride nm.
// The writing sweep recomputes r_z with the same operations on the same operands, so it keeps exactly
// the nodes the counting sweep counted.  Plain vector loads and stores; FP64 VALU only.
//
// k_current_loads: one wave per case, 4 cases per workgroup; the nodes over the lanes in passes of
// 64, each lane's six sums in node order, then a fixed-order xor butterfly: the same bits in every
// lane, and a case's bits do not depend on the cases next to it.
#pragma once
#include "rh_common.h"
#include "rh_pose.h"

namespace rh {

constexpr int kPoseThreads = 256;
constexpr int kPoseChunks = RH_POSE_MAX_NODES / 64;

struct PoseLds {
  double fr[pose::kMembFields][RH_POSE_MAX_MEMBERS];   // rA(3) rB(3) q(3) p1(3) p2(3) l
  unsigned long long mask[kPoseChunks];
  int off[kPoseChunks + 1];
  int mslot[RH_POSE_MAX_MEMBERS];
  int nn, nm;
  unsigned short nmemb_of[RH_POSE_MAX_NODES];
};

__device__ __forceinline__ int pose_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the node -> member map from mstart (clamped: a bad table can misplace nodes, never leave the arrays)
__device__ __forceinline__ void pose_node_members(const int* __restrict__ mstart, int nmemb, int nnode,
                                                  unsigned short* nmemb_of) {
  for (int j = threadIdx.x; j < RH_POSE_MAX_NODES; j += blockDim.x) nmemb_of[j] = 0;
  __syncthreads();
  for (int m = threadIdx.x; m < nmemb; m += blockDim.x) {
    const int a = pose_clamp(mstart[m], nnode), b = pose_clamp(mstart[m + 1], nnode);
    for (int j = a; j < b; ++j) nmemb_of[j] = (unsigned short)m;
  }
}

__device__ __forceinline__ int pose_rank(const PoseLds& S, int j) {
  const int c = j >> 6;
  return S.off[c] + __popcll(S.mask[c] & ((1ull << (j & 63)) - 1ull));
}

__device__ __forceinline__ void pose_load_frame(const PoseLds& S, int m, pose::Frame& f) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f.rA[i] = S.fr[i][m];
    f.rB[i] = S.fr[3 + i][m];
    f.q[i] = S.fr[6 + i][m];
    f.p1[i] = S.fr[9 + i][m];
    f.p2[i] = S.fr[12 + i][m];
  }
}

// grid npose, 256 threads
__global__ __launch_bounds__(kPoseThreads) void k_pose_designs(rh_pose_record rec, int npose,
                                                               const double* __restrict__ Xs,
                                                               double* __restrict__ node_out,
                                                               double* __restrict__ memb_out,
                                                               int* __restrict__ mstart_out, int* __restrict__ nn_out,
                                                               int* __restrict__ nm_out) {
#pragma clang fp contract(off)
  __shared__ PoseLds S;
  const int pose_i = blockIdx.x;
  const int tid = threadIdx.x;
  const int nmemb = rec.nmemb, nnode = rec.nnode;
  const double* __restrict__ nt = rec.node;
  double X[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) X[i] = Xs[(size_t)pose_i * 6 + i];

  // A. member frames and the node -> member map
  pose_node_members(rec.mstart, nmemb, nnode, S.nmemb_of);
  {
    double R[9];
    pose::rotation(X, R);
    for (int m = tid; m < nmemb; m += kPoseThreads) {
      pose::Frame f;
      pose::member_frame(rec.memb, nmemb, m, X, R, f);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        S.fr[i][m] = f.rA[i];
        S.fr[3 + i][m] = f.rB[i];
        S.fr[6 + i][m] = f.q[i];
        S.fr[9 + i][m] = f.p1[i];
        S.fr[12 + i][m] = f.p2[i];
      }
      S.fr[15][m] = rec.memb[pose::kLen * nmemb + m];
    }
  }
  __syncthreads();

  // B. counting sweep
  const int npass = (nnode + kPoseThreads - 1) / kPoseThreads;
  for (int p = 0; p < npass; ++p) {
    const int j = p * kPoseThreads + tid;
    bool wet = false;
    if (j < nnode) {
      const int m = S.nmemb_of[j];
      wet = pose::node_coord(S.fr[2][m], S.fr[5][m], nt[(size_t)RH_NF_T * nnode + j], S.fr[15][m]) < 0.0;
    }
    const unsigned long long b = __ballot(wet);
    if ((tid & 63) == 0) S.mask[j >> 6] = b;
  }
  __syncthreads();

  // C. offsets, kept members, mstart
  if (tid == 0) {
    const int nchunk = npass * (kPoseThreads / 64);
    int acc = 0;
    for (int c = 0; c < nchunk; ++c) {
      S.off[c] = acc;
      acc += __popcll(S.mask[c]);
    }
    S.off[nchunk] = acc;
    int* ms = mstart_out + (size_t)pose_i * (nmemb + 1);
    int nm = 0;
    for (int m = 0; m < nmemb; ++m) {
      const int a = pose_clamp(rec.mstart[m], nnode), b = pose_clamp(rec.mstart[m + 1], nnode);
      const int ra = a < nnode ? pose_rank(S, a) : acc, rb = b < nnode ? pose_rank(S, b) : acc;
      if (rb > ra) {
        S.mslot[m] = nm;
        ms[nm] = ra;
        ++nm;
      } else {
        S.mslot[m] = -1;
      }
    }
    ms[nm] = acc;
    S.nn = acc;
    S.nm = nm;
    nn_out[pose_i] = acc;
    nm_out[pose_i] = nm;
  }
  __syncthreads();
  const int nn = S.nn, nm = S.nm;

  // D. writing sweep: nodes, then members
  double* __restrict__ no = node_out + (size_t)pose_i * RH_NF_COUNT * nnode;
  for (int p = 0; p < npass; ++p) {
    const int j = p * kPoseThreads + tid;
    if (j >= nnode || !((S.mask[j >> 6] >> (j & 63)) & 1ull)) continue;
    const int slot = pose_rank(S, j);
    const int m = S.nmemb_of[j];
    pose::Frame f;
    pose_load_frame(S, m, f);
    const double ls = nt[(size_t)RH_NF_T * nnode + j], l = S.fr[15][m];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double r = pose::node_coord(f.rA[i], f.rB[i], ls, l);
      no[(size_t)(RH_NF_RX + i) * nn + slot] = r;
      no[(size_t)(RH_NF_XX + i) * nn + slot] = r - X[i];
      no[(size_t)(RH_NF_QX + i) * nn + slot] = f.q[i];
      no[(size_t)(RH_NF_P1X + i) * nn + slot] = f.p1[i];
      no[(size_t)(RH_NF_P2X + i) * nn + slot] = f.p2[i];
    }
#pragma unroll
    for (int fld = RH_NF_AQ; fld < RH_NF_COUNT; ++fld)
      no[(size_t)fld * nn + slot] = fld == RH_NF_MCF ? 0.0 : nt[(size_t)fld * nnode + j];
  }
  double* __restrict__ mo = memb_out + (size_t)pose_i * RH_MF_COUNT * nmemb;
  for (int m = tid; m < nmemb; m += kPoseThreads) {
    const int slot = S.mslot[m];
    if (slot < 0) continue;
    pose::Frame f;
    pose_load_frame(S, m, f);
    double col[RH_MF_COUNT];
    pose::member_column(f, X, col);
#pragma unroll
    for (int i = 0; i < RH_MF_COUNT; ++i) mo[(size_t)i * nm + slot] = col[i];
  }
}

// grid ceil(ncase / 4), 256 threads
__global__ __launch_bounds__(kPoseThreads) void k_current_loads(rh_pose_record rec, double x0, double y0, double z0,
                                                                int ncase, const double* __restrict__ speed,
                                                                const double* __restrict__ heading_deg, double depth,
                                                                double Zref, double shearExp, double rho,
                                                                double* __restrict__ D_out) {
#pragma clang fp contract(off)
  __shared__ unsigned short nmemb_of[RH_POSE_MAX_NODES];
  const int nmemb = rec.nmemb, nnode = rec.nnode;
  pose_node_members(rec.mstart, nmemb, nnode, nmemb_of);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (kPoseThreads / 64) + (threadIdx.x >> 6);
  if (c >= ncase) return;   // (a whole wave: no barrier follows)
  const double* __restrict__ nt = rec.node;
  const double* __restrict__ mt = rec.memb;
  const double Xref[3] = {x0, y0, z0};
  const double U = speed[c];
  const double hr = heading_deg[c] * (M_PI / 180.0);   // np.deg2rad
  const double ch = cos(hr), sh = sin(hr);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = lane; j < nnode; j += 64) {
    const int m = nmemb_of[j];
    const double ls = nt[(size_t)RH_NF_T * nnode + j], l = mt[pose::kLen * nmemb + m];
    double r[3], q[3], p1[3], p2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double rA = Xref[i] + mt[(pose::kRA0 + i) * nmemb + m], rB = Xref[i] + mt[(pose::kRB0 + i) * nmemb + m];
      r[i] = pose::node_coord(rA, rB, ls, l);
      q[i] = mt[(pose::kQ0 + i) * nmemb + m];
      p1[i] = mt[(pose::kP10 + i) * nmemb + m];
      p2[i] = mt[(pose::kP20 + i) * nmemb + m];
    }
    if (!(r[2] < 0.0)) continue;
    double D[6];
    pose::current_node_load(r, Xref, q, p1, p2, nt[(size_t)RH_NF_AQ * nnode + j], nt[(size_t)RH_NF_AP1 * nnode + j],
                            nt[(size_t)RH_NF_AP2 * nnode + j], nt[(size_t)RH_NF_AEND * nnode + j],
                            nt[(size_t)RH_NF_CDQ * nnode + j], nt[(size_t)RH_NF_CDP1 * nnode + j],
                            nt[(size_t)RH_NF_CDP2 * nnode + j], nt[(size_t)RH_NF_CDEND * nnode + j],
                            nt[(size_t)RH_NF_CIRC * nnode + j] != 0.0, U, ch, sh, depth, Zref, shearExp, rho, D);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] += D[i];
  }
  // every lane of the wave is here (lanes without a node carry zeros)
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = acc[i];
    for (int mk = 1; mk < 64; mk <<= 1) v += __shfl_xor(v, mk);
    acc[i] = v;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) D_out[(size_t)c * 6 + i] = acc[i];
  }
}

}  // namespace rh

namespace {
int check_pose_record(const rh_pose_record* rec, const char* who) {
  if (!rec) return fail(RH_EINVAL, "%s: null record", who);
  if (rec->nmemb < 1 || rec->nmemb > RH_POSE_MAX_MEMBERS)
    return fail(RH_EINVAL, "%s: nmemb=%d outside [1, %d]", who, rec->nmemb, RH_POSE_MAX_MEMBERS);
  if (rec->nnode < 1 || rec->nnode > RH_POSE_MAX_NODES)
    return fail(RH_EINVAL, "%s: nnode=%d outside [1, %d]", who, rec->nnode, RH_POSE_MAX_NODES);
  if (!rec->memb || !rec->node || !rec->mstart || !rec->mstart_host) return fail(RH_EINVAL, "%s: null record table", who);
  const int* ms = rec->mstart_host;
  if (ms[0] != 0 || ms[rec->nmemb] != rec->nnode)
    return fail(RH_EINVAL, "%s: mstart must run from 0 to nnode=%d", who, rec->nnode);
  for (int m = 0; m < rec->nmemb; ++m)
    if (ms[m + 1] < ms[m]) return fail(RH_EINVAL, "%s: mstart decreases at member %d", who, m);
  return RH_OK;
}
}  // namespace

int rh_pose_designs(rh_ctx* ctx, const rh_pose_record* rec, int npose, const double* X, double* node_out,
                    double* memb_out, int* mstart_out, int* nn_out, int* nm_out, rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_pose_designs: null context");
  if (int r = check_pose_record(rec, "rh_pose_designs")) return r;
  if (npose < 0 || npose > (1 << 20)) return fail(RH_EINVAL, "rh_pose_designs: %d poses outside [0, 2^20]", npose);
  if (npose == 0) return RH_OK;
  if (!X || !node_out || !memb_out || !mstart_out || !nn_out || !nm_out)
    return fail(RH_EINVAL, "rh_pose_designs: null X, node_out, memb_out, mstart_out, nn_out or nm_out");
  RH_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(rh::k_pose_designs, dim3((unsigned)npose), dim3(rh::kPoseThreads), 0, (hipStream_t)stream, *rec,
                     npose, X, node_out, memb_out, mstart_out, nn_out, nm_out);
  RH_HIP(hipGetLastError());
  return RH_OK;
}

int rh_current_loads(rh_ctx* ctx, const rh_pose_record* rec, const double* X_ref, int ncase, const double* speed,
                     const double* heading_deg, double depth, double Zref, double shearExp, double rho, double* D_out,
                     rh_stream stream) {
  if (!ctx) return fail(RH_EINVAL, "rh_current_loads: null context");
  if (int r = check_pose_record(rec, "rh_current_loads")) return r;
  if (!X_ref) return fail(RH_EINVAL, "rh_current_loads: null X_ref");
  if (X_ref[3] != 0.0 || X_ref[4] != 0.0 || X_ref[5] != 0.0)
    return fail(RH_EINVAL, "rh_current_loads: X_ref must be a pure translation (the record's vectors are the pose's)");
  if (!(depth + Zref > 0.0)) return fail(RH_EINVAL, "rh_current_loads: depth + Zref = %g must be > 0", depth + Zref);
  if (ncase < 0 || ncase > (1 << 24)) return fail(RH_EINVAL, "rh_current_loads: %d cases outside [0, 2^24]", ncase);
  if (ncase == 0) return RH_OK;
  if (!speed || !heading_deg || !D_out) return fail(RH_EINVAL, "rh_current_loads: null speed, heading_deg or D_out");
  RH_HIP(hipSetDevice(ctx->device));
  const int per = rh::kPoseThreads / 64;
  hipLaunchKernelGGL(rh::k_current_loads, dim3((unsigned)((ncase + per - 1) / per)), dim3(rh::kPoseThreads), 0,
                     (hipStream_t)stream, *rec, X_ref[0], X_ref[1], X_ref[2], ncase, speed, heading_deg, depth, Zref,
                     shearExp, rho, D_out);
  RH_HIP(hipGetLastError());
  return RH_OK;
}
