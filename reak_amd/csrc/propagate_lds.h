// propagate_lds.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  What the one-wave kernels keep in LDS and in registers: the chain parameters of a joint
// (JointLds, CPack), the per-edge workspaces, the staging of the chain and of the environment shapes.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "rkh_internal.h"

namespace rkh {

struct __attribute__((aligned(16))) JointLds {  // chain parameters of one joint group, staged in LDS
  double axis[3], joint_inertia;
  double axis_n[3], mass;
  double off_pos[3], pad0;
  double off_quat[4];
  double off_R[9], pad1;
  double inertia[6];
};

template <int N>
struct __attribute__((aligned(16))) GroupWs {  // per-edge LDS workspace
  double x[2 * N];                  // state being differentiated (q, qd interleaved)
  double b[2 * N];                  // steer target
  double u[N];                      // held input
  double tmp[2 * N];                // lane-parallel -> sequential-sum staging
  double cs[N][4];                  // c2, s2 (half angle), c1, s1 (full angle)
  double Epos[N][3], Equat[N][4];   // joint end frames (jacobian parents)
  double Lpos[N][3], Lquat[N][4];   // link end frames (inertia frames)
  double FT[N][6];                  // inertia_3D d'Alembert force / torque (to be subtracted)
  double BFT[2][6];                 // flexible beam force / torque on its two anchor frames (zero without a beam)
  double Tcm[N][N][6];              // [body][coord] jacobian column (v, w)
  double Mf[N][N];                  // Tcm^T (Mcm Tcm) before symmetrisation
  double M[N][N];                   // symmetric M, overwritten by its Cholesky factor
  double Rpos[2 * N][3], Rquat[2 * N][4];  // robot shapes, global pose
  // two waves per edge (state_derivative_duo): x' as the solving wave leaves it for the other one, the number of joints
  // whose end frames the first wave has published, the first wave's "pivot below 1e-8" verdict
  double dpx[2 * N];
  double R2[N][9], RA[N][9];               // rotation matrices of the joint rotations (half-angle quaternion / axis-angle form)
  double Wj[N][3], ALj[N][3], ACCj[N][3];  // link end frames: angular velocity, angular acceleration, acceleration
  uint32_t duo_ready, duo_sing;
};

template <int N, int GL>
struct BlockLds {
  JointLds joints[N];
  double base[10];  // pos3, quat4, acc3
  double sink[64][4];  // per-lane dummy store target: keeps the group-leader stores branch-free
  GroupWs<N> g[64 / GL];
};

// the quasi-static kernels (edge walk, distance query) only need what the proximity test touches
template <int N>
struct __attribute__((aligned(16))) GroupWsQs {
  double x[2 * N];
  double tmp[2 * N];
  double cs[N][4];
  double Epos[N][3], Equat[N][4];
  double Rpos[2 * N][3], Rquat[2 * N][4];
};
template <int N, int GL>
struct BlockLdsQs {
  JointLds joints[N];
  double base[10];
  double sink[64][4];
  GroupWsQs<N> g[64 / GL];
};

RKH_DI d3 ld3(const double* p) { return d3{p[0], p[1], p[2]}; }
RKH_DI d4 ld4(const double* p) { return d4{p[0], p[1], p[2], p[3]}; }
RKH_DI void st3(double* p, d3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
RKH_DI void st4(double* p, d4 v) { p[0] = v.w; p[1] = v.x; p[2] = v.y; p[3] = v.z; }
RKH_DI m33 ldm(const double* p) { return m33{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }

// Chain parameters are wave-uniform.  They are packed into R vector registers (lane l of register r
// holds flat parameter r*64 + l, JointLds layout) and read back with v_readlane: no memory latency on
// the serial sweeps' critical path and no long-lived scalar registers.
template <int N>
struct CPack {
  static constexpr int R = (N * 32 + 63) / 64;
  double v[R];
};
RKH_DI double readlane_f64(double v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
template <int N>
RKH_DI double cget(const CPack<N>& cp, int idx) { return readlane_f64(cp.v[idx >> 6], idx & 63); }
template <int N>
RKH_DI d3 cget3(const CPack<N>& cp, int idx) { return d3{cget(cp, idx), cget(cp, idx + 1), cget(cp, idx + 2)}; }
template <int N>
RKH_DI CPack<N> load_cpack(const JointLds* jl, int lane) {
  CPack<N> cp;
#pragma unroll
  for (int r = 0; r < CPack<N>::R; ++r) {
    const int idx = r * 64 + lane;
    cp.v[r] = idx < N * 32 ? reinterpret_cast<const double*>(jl)[idx] : 0.0;
  }
  return cp;
}
// field offsets inside JointLds (in doubles)
enum : int { JC_AXIS = 0, JC_JIN = 3, JC_AXISN = 4, JC_MASS = 7, JC_OFFP = 8, JC_OFFQ = 12, JC_OFFR = 16, JC_INER = 26 };

template <int N>
__device__ __forceinline__ void stage_chain(const SceneDev* __restrict__ sc, JointLds* jl, double* base, int lane) {
  for (int i = lane; i < N * 32; i += 64) {
    const int j = i >> 5, k = i & 31;
    const JointDev& J = sc->joints[j];
    double v = 0.0;
    if (k < 3) v = J.axis[k];
    else if (k == 3) v = J.joint_inertia;
    else if (k < 7) v = J.axis_n[k - 4];
    else if (k == 7) v = J.mass;
    else if (k < 11) v = J.off_pos[k - 8];
    else if (k == 11) v = 0.0;
    else if (k < 16) v = J.off_quat[k - 12];
    else if (k < 25) v = J.off_R[k - 16];
    else if (k == 25) v = 0.0;
    else v = J.inertia[k - 26];
    reinterpret_cast<double*>(&jl[j])[k] = v;
  }
  if (lane < 3) base[lane] = sc->base_pos[lane];
  else if (lane < 7) base[lane] = sc->base_quat[lane - 3];
  else if (lane < 10) base[lane] = sc->base_acc[lane - 7];
}

__device__ __forceinline__ void stage_env(const SceneDev* __restrict__ sc, ShapeDev* env_lds, int lane) {
  const int n_words = sc->n_env * int(sizeof(ShapeDev) / sizeof(double));
  const double* src = reinterpret_cast<const double*>(sc->env);
  double* dst = reinterpret_cast<double*>(env_lds);
  for (int i = lane; i < n_words; i += 64) dst[i] = src[i];
}

template <int N, int GL>
struct SmemLayoutQs {
  static constexpr size_t block_bytes = (sizeof(BlockLdsQs<N, GL>) + 15) / 16 * 16;
  static size_t bytes(int n_env) { return block_bytes + size_t(n_env) * sizeof(ShapeDev); }
};
template <int N, int GL>
struct SmemLayout {
  static constexpr size_t block_bytes = (sizeof(BlockLds<N, GL>) + 15) / 16 * 16;
  static size_t bytes(int n_env) { return block_bytes + size_t(n_env) * sizeof(ShapeDev); }
};

// exact left-to-right euclidean metric of a lane-distributed difference vector
// (vect_distance_metrics.hpp:126-137): stage the squares in LDS, every lane sums them in order
template <int N>
RKH_DI double group_norm(GroupWs<N>& ws, double diff, int gl) {
  if (gl < 2 * N) ws.tmp[gl] = diff * diff;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 2 * N; ++d) s = s + ws.tmp[d];
  __syncthreads();
  return sqrt(s);
}

}  // namespace rkh
