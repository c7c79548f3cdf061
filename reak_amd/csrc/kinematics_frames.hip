// kinematics_frames.hip -- rkh_direct_kinematics[_2d], rkh_jacobians[_2d] and rkh_inverse_kinematics (include/rkh.h):
// the frames, twists and Jacobians of a KTE chain handed out, and batched damped least-squares pose IK on top of them.
// A module of its own: no existing kernel is touched.  The arithmetic is kinematics_device.h's.
//
// Mapping.
//   kinematics_frames_kernel / kinematics_frames_planar_kernel: one lane per (state, asked frame); a block of 64 lanes
//   serves 64 states of ONE frame, so the frame's place in the chain, the joints on the way and every scene constant are
//   uniform over the wave (scalar loads, uniform branches).  The lane walks base -> frame once for the pose and rates; if
//   Jacobians are asked it walks a second time and writes the column of every upstream joint as it passes the joint's end
//   frame.  Nothing is kept per joint: no LDS, no private array, whatever the chain length -- a chain of 12 joints runs
//   the code a pendulum runs.  The price is the second walk (its sincos again); the columns dominate as soon as a
//   frame has more than a few upstream joints.  Columns of joints that are not upstream are never written: the launcher
//   clears the two arrays first, which is the reference's "start from a nil matrix".
//   kinematics_ik_kernel: one lane per solve.  Per iteration one walk, which leaves the world position and world axis of
//   every upstream joint in LDS ([slot][lane], 8 n doubles per lane with q and dq), then A = J J^T + damping^2 I is summed
//   column by column from those, the 6 x 6 Cholesky solve runs in registers, and dq = J^T y recomputes each column
//   instead of keeping J.  Lanes that have stopped idle until the wave is done.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "kinematics_device.h"
#include "rkh_internal.h"
#include "staged_call.h"

namespace rkh {
namespace {

constexpr int kKinThreads = 64;

struct KinOut {  // device pointers, any may be null
  double* pos;
  double* rot;  // quat[4] / (cos, sin)
  double* vel;
  double* ang_vel;
  double* jac;
  double* jac_dot;
};

// VEL: rates are asked for and given
template <bool VEL>
__global__ __launch_bounds__(kKinThreads) void kinematics_frames_kernel(const KinChain* __restrict__ C,
                                                                        const KinFrameRef* __restrict__ refs,
                                                                        const double* __restrict__ q,
                                                                        const double* __restrict__ qd, uint32_t B, uint32_t F,
                                                                        uint32_t blocks_b, KinOut out) {
  const uint32_t fi = blockIdx.x / blocks_b;
  const uint32_t b = (blockIdx.x % blocks_b) * kKinThreads + threadIdx.x;
  if (b >= B) return;
  const KinFrameRef ref = refs[fi];
  const int n = C->n_dof;
  const double* qb = q + size_t(b) * n;
  const double* qdb = (VEL && qd) ? qd + size_t(b) * n : nullptr;
  const KinFrame T = kin_walk<VEL>(*C, ref, qb, qdb, 1, [](int, const KinFrame&) {});
  const size_t slot = size_t(b) * F + fi;
  if (out.pos) { out.pos[3 * slot] = T.p.x; out.pos[3 * slot + 1] = T.p.y; out.pos[3 * slot + 2] = T.p.z; }
  if (out.rot) { out.rot[4 * slot] = T.Q.w; out.rot[4 * slot + 1] = T.Q.x; out.rot[4 * slot + 2] = T.Q.y; out.rot[4 * slot + 3] = T.Q.z; }
  if (out.vel) { out.vel[3 * slot] = T.v.x; out.vel[3 * slot + 1] = T.v.y; out.vel[3 * slot + 2] = T.v.z; }
  if (out.ang_vel) { out.ang_vel[3 * slot] = T.w.x; out.ang_vel[3 * slot + 1] = T.w.y; out.ang_vel[3 * slot + 2] = T.w.z; }
  if (!out.jac && !out.jac_dot) return;
  const m33 RT = rotmat(T.Q);
  const d3 WT = mul(RT, T.w);
  double* jac = out.jac ? out.jac + slot * 6 * n : nullptr;
  double* jdot = out.jac_dot ? out.jac_dot + slot * 6 * n : nullptr;
  kin_walk<VEL>(*C, ref, qb, qdb, 1, [&](int j, const KinFrame& E) {
    if (!((ref.up >> j) & 1u)) return;
    const KinJoint& J = C->joints[j];
    const KinCol c = kin_column<VEL>(J.prismatic != 0, kin_ld3(J.axis), E, T, RT, WT);
    if (jac) {
      jac[j] = c.v.x; jac[n + j] = c.v.y; jac[2 * n + j] = c.v.z;
      jac[3 * n + j] = c.w.x; jac[4 * n + j] = c.w.y; jac[5 * n + j] = c.w.z;
    }
    if (jdot) {
      jdot[j] = c.vd.x; jdot[n + j] = c.vd.y; jdot[2 * n + j] = c.vd.z;
      jdot[3 * n + j] = c.wd.x; jdot[4 * n + j] = c.wd.y; jdot[5 * n + j] = c.wd.z;
    }
  });
}

template <bool VEL>
__global__ __launch_bounds__(kKinThreads) void kinematics_frames_planar_kernel(const KinChain* __restrict__ C,
                                                                               const KinFrameRef* __restrict__ refs,
                                                                               const double* __restrict__ q,
                                                                               const double* __restrict__ qd, uint32_t B,
                                                                               uint32_t F, uint32_t blocks_b, KinOut out) {
  const uint32_t fi = blockIdx.x / blocks_b;
  const uint32_t b = (blockIdx.x % blocks_b) * kKinThreads + threadIdx.x;
  if (b >= B) return;
  const KinFrameRef ref = refs[fi];
  const int n = C->n_dof;
  const double* qb = q + size_t(b) * n;
  const double* qdb = (VEL && qd) ? qd + size_t(b) * n : nullptr;
  const KinFrame2 T = kin_walk2<VEL>(*C, ref, qb, qdb, 1, [](int, const KinFrame2&) {});
  const size_t slot = size_t(b) * F + fi;
  if (out.pos) { out.pos[2 * slot] = T.p.x; out.pos[2 * slot + 1] = T.p.y; }
  if (out.rot) { out.rot[2 * slot] = T.R.x; out.rot[2 * slot + 1] = T.R.y; }
  if (out.vel) { out.vel[2 * slot] = T.v.x; out.vel[2 * slot + 1] = T.v.y; }
  if (out.ang_vel) out.ang_vel[slot] = T.w;
  if (!out.jac && !out.jac_dot) return;
  double* jac = out.jac ? out.jac + slot * 3 * n : nullptr;
  double* jdot = out.jac_dot ? out.jac_dot + slot * 3 * n : nullptr;
  kin_walk2<VEL>(*C, ref, qb, qdb, 1, [&](int j, const KinFrame2& E) {
    if (!((ref.up >> j) & 1u)) return;
    const KinJoint& J = C->joints[j];
    const KinCol2 c = kin_column2<VEL>(J.prismatic != 0, kin_ld2(J.axis), E, T);
    if (jac) { jac[j] = c.v.x; jac[n + j] = c.v.y; jac[2 * n + j] = c.w; }
    if (jdot) { jdot[j] = c.vd.x; jdot[n + j] = c.vd.y; jdot[2 * n + j] = 0.0; }
  });
}

// ---- pose IK ---------------------------------------------------------------------------------------------------------
struct IkOut {
  double* q;         // [solves][n]
  double* x;         // [solves][2 n]: (q, 0) interleaved, the states of the distance query that follows
  double* res_pos;   // [solves]
  double* res_rot;
  uint32_t* iters;
  uint32_t* flags;   // bit 0: converged
};
struct IkDev {  // one call's constants, on the device
  KinFrameRef ref;
  uint32_t max_iters;
  double damping2, max_step, tol_pos, tol_rot;
  double lower[kKinMaxDof], upper[kKinMaxDof];
  IkOut out;  // read when a lane is done: six pointers that need not stay in scalar registers over the iteration
};
// a wave-uniform value the iteration reads all the time, kept in a vector register: the scalar file is the scarce one here
__device__ __forceinline__ double in_vgpr(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// LDS per lane: 8 n doubles as [slot][lane]: q (n), dq (n), the upstream joints' end positions (3 n) and world axes (3 n)
__global__ __launch_bounds__(kKinThreads) void kinematics_ik_kernel(const KinChain* __restrict__ C, const IkDev* __restrict__ P,
                                                                    const rkh_pose* __restrict__ targets,
                                                                    const double* __restrict__ seeds, uint32_t n_solves,
                                                                    uint32_t S) {
  extern __shared__ double ik_lds[];
  const int lane = threadIdx.x;
  const uint32_t sidx = blockIdx.x * kKinThreads + lane;
  if (sidx >= n_solves) return;  // no barrier below: every lane works on its own LDS column
  const int n = C->n_dof;
  double* qs = ik_lds + lane;                        // q[j] at qs[j * 64]
  double* dqs = ik_lds + size_t(n) * kKinThreads + lane;
  double* pj = ik_lds + size_t(2 * n) * kKinThreads + lane;  // p_j component c at pj[(3 j + c) * 64]
  double* aj = ik_lds + size_t(5 * n) * kKinThreads + lane;
  const KinFrameRef ref = P->ref;
  const rkh_pose tg = targets[sidx / S];
  const d3 pstar = kin_ld3(tg.pos);
  const d4 Qstar = kin_ld4(tg.quat);
  for (int j = 0; j < n; ++j) qs[j * kKinThreads] = kin_clamp(seeds[size_t(sidx) * n + j], P->lower[j], P->upper[j]);
  const uint32_t max_iters = P->max_iters;
  const double tol_pos = in_vgpr(P->tol_pos), tol_rot = in_vgpr(P->tol_rot), max_step = in_vgpr(P->max_step),
               damping2 = in_vgpr(P->damping2);
  double rp = 0.0, rr = 0.0;
  uint32_t k = 0, conv = 0;
  for (;; ++k) {
    const KinFrame T = kin_walk<false>(*C, ref, qs, nullptr, kKinThreads, [&](int j, const KinFrame& E) {
      const d3 A = mul(rotmat(E.Q), kin_ld3(C->joints[j].axis));
      pj[(3 * j) * kKinThreads] = E.p.x; pj[(3 * j + 1) * kKinThreads] = E.p.y; pj[(3 * j + 2) * kKinThreads] = E.p.z;
      aj[(3 * j) * kKinThreads] = A.x; aj[(3 * j + 1) * kKinThreads] = A.y; aj[(3 * j + 2) * kKinThreads] = A.z;
    });
    double e[6];
    kin_pose_error(T, pstar, Qstar, e);
    rp = sqrt(((0.0 + e[0] * e[0]) + e[1] * e[1]) + e[2] * e[2]);
    rr = sqrt(((0.0 + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5]);
    if (rp <= tol_pos && rr <= tol_rot) {
      conv = 1;
      break;
    }
    if (k == max_iters) break;
    const m33 RT = rotmat(T.Q);
    // column of joint j in the frame's coordinates, from what the walk left in LDS
    auto column = [&](int j, double* c) {
      const d3 A = mk3(aj[(3 * j) * kKinThreads], aj[(3 * j + 1) * kKinThreads], aj[(3 * j + 2) * kKinThreads]);
      const bool prism = C->joints[j].prismatic != 0;
      const d3 d = T.p - mk3(pj[(3 * j) * kKinThreads], pj[(3 * j + 1) * kKinThreads], pj[(3 * j + 2) * kKinThreads]);
      const d3 v = mulT(prism ? A : cross(A, d), RT);
      const d3 w = prism ? mk3(0.0, 0.0, 0.0) : mulT(A, RT);
      c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = w.x; c[4] = w.y; c[5] = w.z;
    };
    double Am[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) Am[i] = 0.0;
    for (int j = ref.first; j <= ref.last; ++j) {
      if (!((ref.up >> j) & 1u)) continue;
      double c[6];
      column(j, c);
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int cc = 0; cc <= r; ++cc) Am[r * (r + 1) / 2 + cc] = Am[r * (r + 1) / 2 + cc] + c[r] * c[cc];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) Am[r * (r + 1) / 2 + r] = Am[r * (r + 1) / 2 + r] + damping2;
    if (!kin_cholesky6(Am, e)) break;  // not positive definite to rounding: stop, not converged
    double mx = 0.0;
    for (int j = 0; j < n; ++j) {
      double dq = 0.0;
      if (j >= ref.first && j <= ref.last && ((ref.up >> j) & 1u)) {
        double c[6];
        column(j, c);
#pragma unroll
        for (int r = 0; r < 6; ++r) dq = dq + c[r] * e[r];
      }
      dqs[j * kKinThreads] = dq;
      const double a = fabs(dq);
      if (a > mx) mx = a;
    }
    const bool scale = mx > max_step;
    const double sc = scale ? max_step / mx : 1.0;
    for (int j = 0; j < n; ++j) {
      const double dq = scale ? dqs[j * kKinThreads] * sc : dqs[j * kKinThreads];
      qs[j * kKinThreads] = kin_clamp(qs[j * kKinThreads] + dq, P->lower[j], P->upper[j]);
    }
  }
  const IkOut out = P->out;
  for (int j = 0; j < n; ++j) {
    const double v = qs[j * kKinThreads];
    out.q[size_t(sidx) * n + j] = v;
    out.x[size_t(sidx) * 2 * n + 2 * j] = v;
    out.x[size_t(sidx) * 2 * n + 2 * j + 1] = 0.0;
  }
  out.res_pos[sidx] = rp;
  out.res_rot[sidx] = rr;
  out.iters[sidx] = k;
  out.flags[sidx] = conv;
}

rkh_status kind_supported(const rkh_scene* scene, bool planar_entry, const char* who) {
  if ((scene->host.planar != 0) == planar_entry) return RKH_OK;
  set_error(std::string(who) + (planar_entry ? ": not supported for 3D scenes: their frames come from the entries without _2d"
                                             : ": not supported for planar (2D) scenes: their frames come from the _2d entries"));
  return RKH_ERR_UNSUPPORTED;
}

rkh_status frame_refs(const rkh_scene* scene, const int32_t* frames, uint32_t F, const char* who, std::vector<KinFrameRef>* refs) {
  refs->resize(F);
  for (uint32_t f = 0; f < F; ++f) {
    const int32_t id = frames[f];
    if (id < 0 || size_t(id) >= scene->frame_table.size() || scene->frame_table[id].kind == KIN_INVALID) {
      set_error(std::string(who) + ": frame " + std::to_string(id) + " is not a frame of the chain");
      return RKH_ERR_BAD_ARG;
    }
    (*refs)[f] = scene->frame_table[id];
  }
  return RKH_OK;
}

// All four frame entries: checks, transfers, the clear of the Jacobian arrays, one launch.  ms != null: the launch (with
// its clear) is repeated `runs` times between events after this first one (rkh_diag_kinematics_ms).
rkh_status frames_run(const char* who, bool planar_entry, rkh_scene* scene, const double* q, const double* qd, uint32_t B,
                      const int32_t* frames, uint32_t F, double* pos, double* rot, double* vel, double* ang_vel, double* jac,
                      double* jac_dot, uint32_t runs, float* ms) {
  if (!scene) return RKH_ERR_BAD_ARG;
  RKH_TRY(kind_supported(scene, planar_entry, who));
  if (B == 0 || F == 0) return RKH_OK;
  if (!q || !frames) {
    set_error(std::string(who) + ": q and frames must not be NULL");
    return RKH_ERR_BAD_ARG;
  }
  if (!pos && !rot && !vel && !ang_vel && !jac && !jac_dot) {
    set_error(std::string(who) + ": every output pointer is NULL");
    return RKH_ERR_BAD_ARG;
  }
  std::vector<KinFrameRef> refs;
  RKH_TRY(frame_refs(scene, frames, F, who, &refs));
  const int n = scene->host.n_dof;
  const uint32_t blocks_b = (B + kKinThreads - 1) / kKinThreads;
  if (uint64_t(blocks_b) * F > 0x7FFFFFFFull) {
    set_error(std::string(who) + ": too many (state, frame) pairs for one launch");
    return RKH_ERR_CAPACITY;
  }
  const int pd = planar_entry ? 2 : 3, rd = planar_entry ? 2 : 4, wd = planar_entry ? 1 : 3, rows = planar_entry ? 3 : 6;
  const size_t slots = size_t(B) * F;
  hipStream_t s = scene->ctx->stream;
  RKH_HIP(hipSetDevice(scene->ctx->device));
  StagedCall call(s);  // (refs was declared before it)
  const double* d_q = call.in(q, size_t(B) * n);
  const double* d_qd = qd ? call.in(qd, size_t(B) * n) : nullptr;
  const KinFrameRef* d_refs = call.in(refs.data(), F);
  KinOut out;
  out.pos = pos ? call.out(pos, slots * pd) : nullptr;
  out.rot = rot ? call.out(rot, slots * rd) : nullptr;
  out.vel = vel ? call.out(vel, slots * pd) : nullptr;
  out.ang_vel = ang_vel ? call.out(ang_vel, slots * wd) : nullptr;
  out.jac = jac ? call.out(jac, slots * rows * n) : nullptr;
  out.jac_dot = jac_dot ? call.out(jac_dot, slots * rows * n) : nullptr;
  RKH_TRY(call.status());
  // NULL qd = zero rates: the walk then carries zeros for the rates, and JacDot is the clear below
  const bool rates = qd && (vel || ang_vel || jac_dot);
  auto launch = [&]() -> rkh_status {
    if (jac) RKH_HIP(hipMemsetAsync(out.jac, 0, slots * rows * n * 8, s));
    if (jac_dot) RKH_HIP(hipMemsetAsync(out.jac_dot, 0, slots * rows * n * 8, s));
    const dim3 grid(blocks_b * F), block(kKinThreads);
    if (planar_entry) {
      if (rates) hipLaunchKernelGGL(kinematics_frames_planar_kernel<true>, grid, block, 0, s, scene->d_kin.get(), d_refs, d_q, d_qd, B, F, blocks_b, out);
      else hipLaunchKernelGGL(kinematics_frames_planar_kernel<false>, grid, block, 0, s, scene->d_kin.get(), d_refs, d_q, (const double*)nullptr, B, F, blocks_b, out);
    } else {
      if (rates) hipLaunchKernelGGL(kinematics_frames_kernel<true>, grid, block, 0, s, scene->d_kin.get(), d_refs, d_q, d_qd, B, F, blocks_b, out);
      else hipLaunchKernelGGL(kinematics_frames_kernel<false>, grid, block, 0, s, scene->d_kin.get(), d_refs, d_q, (const double*)nullptr, B, F, blocks_b, out);
    }
    RKH_HIP(hipGetLastError());
    return RKH_OK;
  };
  RKH_TRY(launch());
  if (ms) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (auto& e : ev) RKH_HIP(hipEventCreate(&e));
    rkh_status st = RKH_OK;
    for (uint32_t r = 0; st == RKH_OK && r < runs; ++r) {
      hipError_t e = hipEventRecord(ev[0], s);
      if (e == hipSuccess) st = launch();
      if (e == hipSuccess) e = hipEventRecord(ev[1], s);
      if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms[r], ev[0], ev[1]);
      if (e != hipSuccess && st == RKH_OK) {
        set_error(std::string(who) + ": " + hipGetErrorString(e));
        st = RKH_ERR_DEVICE;
      }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    RKH_TRY(st);
  }
  return call.fetch();
}

// rkh_inverse_kinematics; ms != null: the solve launch and the distance launch are repeated `runs` times between events
// after the first ones, ms[r][0] = solves, ms[r][1] = distance query (rkh_diag_ik_ms)
rkh_status ik_run(const char* who, rkh_scene* scene, int32_t frame, const rkh_pose* targets, uint32_t T, const double* seeds,
                  uint32_t S, const double* lower, const double* upper, const rkh_ik_params* prm, double* q_out,
                  double* res_pos, double* res_rot, uint32_t* iters, uint32_t* flags, uint32_t* best, uint32_t runs, float* ms) {
  if (!scene || !prm) return RKH_ERR_BAD_ARG;
  RKH_TRY(kind_supported(scene, false, who));
  if (prm->struct_size != sizeof(rkh_ik_params)) {
    set_error(std::string(who) + ": rkh_ik_params.struct_size is " + std::to_string(prm->struct_size) + ", this library's is " +
              std::to_string(sizeof(rkh_ik_params)));
    return RKH_ERR_BAD_ARG;
  }
  if (!(prm->damping > 0.0) || !(prm->max_step > 0.0) || !(prm->tol_pos >= 0.0) || !(prm->tol_rot >= 0.0) ||
      !std::isfinite(prm->damping) || !std::isfinite(prm->max_step)) {
    set_error(std::string(who) + ": damping and max_step must be positive and finite, the tolerances not negative");
    return RKH_ERR_BAD_ARG;
  }
  if (!lower || !upper) return RKH_ERR_BAD_ARG;
  const int n = scene->host.n_dof;
  for (int j = 0; j < n; ++j)
    if (!(lower[j] <= upper[j])) {
      set_error(std::string(who) + ": lower[" + std::to_string(j) + "] > upper[" + std::to_string(j) + "] (or not a number)");
      return RKH_ERR_BAD_ARG;
    }
  std::vector<KinFrameRef> refs;
  RKH_TRY(frame_refs(scene, &frame, 1, who, &refs));
  if (T == 0 || S == 0) return RKH_OK;
  if (!targets || !seeds || !q_out) {
    set_error(std::string(who) + ": targets, seeds and q_out must not be NULL");
    return RKH_ERR_BAD_ARG;
  }
  for (uint32_t t = 0; t < T; ++t) {
    double nn = 0.0;
    bool finite = true;
    for (int i = 0; i < 4; ++i) nn += targets[t].quat[i] * targets[t].quat[i], finite = finite && std::isfinite(targets[t].quat[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(targets[t].pos[i]);
    if (!finite || !(std::fabs(std::sqrt(nn) - 1.0) <= 1e-9)) {
      set_error(std::string(who) + ": target " + std::to_string(t) + " is not finite or its quaternion is not unit (to 1e-9)");
      return RKH_ERR_BAD_ARG;
    }
  }
  const uint64_t n_solves64 = uint64_t(T) * S;
  if (n_solves64 > 0x7FFFFFFFull / 64) {
    set_error(std::string(who) + ": too many solves for one launch");
    return RKH_ERR_CAPACITY;
  }
  const uint32_t N = uint32_t(n_solves64);
  for (size_t k = 0; k < size_t(N) * n; ++k)
    if (!std::isfinite(seeds[k])) {
      set_error(std::string(who) + ": a seed has a coordinate that is not finite");
      return RKH_ERR_BAD_ARG;
    }
  IkDev P;
  std::memset(&P, 0, sizeof(P));
  P.ref = refs[0];
  P.max_iters = prm->max_iters;
  P.damping2 = prm->damping * prm->damping;
  P.max_step = prm->max_step;
  P.tol_pos = prm->tol_pos;
  P.tol_rot = prm->tol_rot;
  for (int j = 0; j < n; ++j) P.lower[j] = lower[j], P.upper[j] = upper[j];
  hipStream_t s = scene->ctx->stream;
  RKH_HIP(hipSetDevice(scene->ctx->device));
  const bool has_pairs = scene->n_pairs > 0;
  std::vector<double> dist(N, INFINITY);  // a scene without pairs: free
  std::vector<uint32_t> fl(N);
  DeviceBuffer<IkDev> d_P;  // uploaded once the arrays it points to exist
  RKH_TRY(d_P.alloc(1));
  StreamWait d_P_idle{s};
  StagedCall call(s);
  const rkh_pose* d_tg = call.in(targets, T);
  const double* d_seeds = call.in(seeds, size_t(N) * n);
  IkOut& out = P.out;
  out.q = call.out(q_out, size_t(N) * n);
  out.x = call.scratch<double>(size_t(N) * 2 * n);
  out.res_pos = call.out(res_pos, N);
  out.res_rot = call.out(res_rot, N);
  out.iters = call.out(iters, N);
  out.flags = call.out(fl.data(), N);
  double* d_dist = call.out(has_pairs ? dist.data() : nullptr, N);
  RKH_TRY(call.status());
  RKH_HIP(hipMemcpyAsync(d_P.get(), &P, sizeof(P), hipMemcpyHostToDevice, s));
  const size_t lds = size_t(8) * n * kKinThreads * sizeof(double);  // at most 48 KB (12 joints)
  auto launch_solve = [&]() -> rkh_status {
    hipLaunchKernelGGL(kinematics_ik_kernel, dim3((N + kKinThreads - 1) / kKinThreads), dim3(kKinThreads), lds, s,
                       scene->d_kin.get(), d_P.get(), d_tg, d_seeds, N, S);
    RKH_HIP(hipGetLastError());
    return RKH_OK;
  };
  auto launch_dist = [&]() -> rkh_status {
    return has_pairs ? launch_min_distance(s, *scene, out.x, N, d_dist) : RKH_OK;
  };
  RKH_TRY(launch_solve());
  RKH_TRY(launch_dist());
  if (ms) {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (auto& e : ev) RKH_HIP(hipEventCreate(&e));
    rkh_status st = RKH_OK;
    for (uint32_t r = 0; st == RKH_OK && r < runs; ++r) {
      hipError_t e = hipEventRecord(ev[0], s);
      if (e == hipSuccess) st = launch_solve();
      if (e == hipSuccess) e = hipEventRecord(ev[1], s);
      if (e == hipSuccess && st == RKH_OK) st = launch_dist();
      if (e == hipSuccess) e = hipEventRecord(ev[2], s);
      if (e == hipSuccess) e = hipEventSynchronize(ev[2]);
      for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms[size_t(r) * 2 + k], ev[k], ev[k + 1]);
      if (e != hipSuccess && st == RKH_OK) {
        set_error(std::string(who) + ": " + hipGetErrorString(e));
        st = RKH_ERR_DEVICE;
      }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    RKH_TRY(st);
  }
  RKH_TRY(call.fetch());
  for (uint32_t k = 0; k < N; ++k) fl[k] = (fl[k] & 1u) | (dist[k] > 0.0 ? 2u : 0u);  // a scene without pairs: free
  if (flags) std::memcpy(flags, fl.data(), size_t(N) * 4);
  if (best)
    for (uint32_t t = 0; t < T; ++t) {
      best[t] = 0xFFFFFFFFu;
      for (uint32_t si = 0; si < S && best[t] == 0xFFFFFFFFu; ++si)
        if (fl[size_t(t) * S + si] == 3u) best[t] = si;
    }
  return RKH_OK;
}

}  // namespace
}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_direct_kinematics(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                 uint32_t F, double* pos, double* quat, double* vel, double* ang_vel) {
  return frames_run("rkh_direct_kinematics", false, scene, q, qd, B, frames, F, pos, quat, vel, ang_vel, nullptr, nullptr, 0, nullptr);
}

rkh_status rkh_direct_kinematics_2d(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                    uint32_t F, double* pos, double* rot, double* vel, double* ang_vel) {
  return frames_run("rkh_direct_kinematics_2d", true, scene, q, qd, B, frames, F, pos, rot, vel, ang_vel, nullptr, nullptr, 0, nullptr);
}

rkh_status rkh_jacobians(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames, uint32_t F,
                         double* jac, double* jac_dot) {
  return frames_run("rkh_jacobians", false, scene, q, qd, B, frames, F, nullptr, nullptr, nullptr, nullptr, jac, jac_dot, 0, nullptr);
}

rkh_status rkh_jacobians_2d(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames, uint32_t F,
                            double* jac, double* jac_dot) {
  return frames_run("rkh_jacobians_2d", true, scene, q, qd, B, frames, F, nullptr, nullptr, nullptr, nullptr, jac, jac_dot, 0, nullptr);
}

rkh_status rkh_inverse_kinematics(rkh_scene* scene, int32_t frame, const rkh_pose* targets, uint32_t T, const double* seeds,
                                  uint32_t S, const double* lower, const double* upper, const rkh_ik_params* params,
                                  double* q_out, double* res_pos, double* res_rot, uint32_t* iters, uint32_t* flags,
                                  uint32_t* best) {
  return ik_run("rkh_inverse_kinematics", scene, frame, targets, T, seeds, S, lower, upper, params, q_out, res_pos, res_rot,
                iters, flags, best, 0, nullptr);
}

rkh_status rkh_diag_kinematics_ms(rkh_scene* scene, const double* q, const double* qd, uint32_t B, const int32_t* frames,
                                  uint32_t F, uint32_t runs, float* ms) {
  if (!scene || !q || !frames || !ms || B == 0 || F == 0 || runs == 0) return RKH_ERR_BAD_ARG;
  const bool planar = scene->host.planar != 0;
  const size_t slots = size_t(B) * F, n = size_t(scene->host.n_dof);
  std::vector<double> pos(slots * 3), rot(slots * 4), vel(slots * 3), w(slots * 3), jac(slots * 6 * n), jdot(slots * 6 * n);
  return frames_run("rkh_diag_kinematics_ms", planar, scene, q, qd, B, frames, F, pos.data(), rot.data(), vel.data(), w.data(),
                    jac.data(), jdot.data(), runs, ms);
}

rkh_status rkh_diag_ik_ms(rkh_scene* scene, int32_t frame, const rkh_pose* targets, uint32_t T, const double* seeds, uint32_t S,
                          const double* lower, const double* upper, const rkh_ik_params* params, uint32_t runs, float* ms) {
  if (!scene || !ms || T == 0 || S == 0 || runs == 0) return RKH_ERR_BAD_ARG;
  std::vector<double> q(size_t(T) * S * size_t(scene->host.n_dof));
  return ik_run("rkh_diag_ik_ms", scene, frame, targets, T, seeds, S, lower, upper, params, q.data(), nullptr, nullptr, nullptr,
                nullptr, nullptr, runs, ms);
}

}  // extern "C"
