// kinematics_host.cpp -- reak_amd/csrc/kinematics_device.h read by a host compiler (through the stand-in for
// <hip/hip_runtime.h> in tests/cpp/hip_host) and checked against values worked out by hand.  A program of its own: built
// with -fsanitize=address,undefined and run by tests/test_kinematics_cpu.py.
//
// The chains (base at the origin, identity orientation):
//   A  two revolute joints about z, links (1, 0, 0) and (0.5, 0, 0): the planar 2R arm in 3D.  At q = (pi/2, pi/2) the
//      first link end is (0, 1, 0), the tip (-0.5, 1, 0), both turned by pi about z at the tip.  With rates (1, 2):
//      tip velocity = w1 z x tip + w2 z x (tip - elbow) = (-1, -0.5, 0) + (0, -1, 0) = (-1, -1.5, 0), angular velocity
//      (0, 0, 3); the tip's columns in ITS coordinates (R = rot(z, pi): x -> -x, y -> -y): joint 0: z x tip = (-1, -0.5, 0)
//      -> (1, 0.5, 0); joint 1: z x (tip - elbow) = (0, -0.5, 0) -> (0, 0.5, 0); both w = (0, 0, 1).
//   B  a prismatic joint along the non-unit axis (0, 2, 0) with link (0, 0, 1), then a revolute joint about x with link
//      (0, 0, 1).  At q = (0.25, pi/2): slider end (0, 0.5, 0), its link end (0, 0.5, 1), tip = that + rot(x, pi/2)(0, 0, 1) =
//      (0, -0.5, 1).  Columns of the tip in its coordinates (R^T v, R = rot(x, pi/2): R^T (x, y, z) = (x, z, -y)):
//      prismatic (0, 2, 0) -> (0, 0, -2), w = 0; revolute: x x (0, -1, 0) = (0, 0, -1) -> (0, -1, 0), w = (1, 0, 0).
//   C  the planar forms of A (revolute_joint_2D) and of B's slider (prismatic_joint_2D along (0, 2)).
//   and the 6 x 6 Cholesky solve on diag(1..6) + a rank-one term, against a residual.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../reak_amd/csrc/kinematics_device.h"

using namespace rkh;

static int g_fail = 0;
static void near(const char* what, double got, double want, double tol = 1e-15) {
  if (!(std::fabs(got - want) <= tol)) {
    std::printf("FAIL %s: got %.17g, want %.17g\n", what, got, want);
    ++g_fail;
  }
}
// pi / 2 is not a double: cos(pi/2) leaves 6e-17, which the chains above multiply by lengths and rates of a few units
static void near3(const char* what, d3 got, double x, double y, double z, double tol = 2e-15) {
  near(what, got.x, x, tol);
  near(what, got.y, y, tol);
  near(what, got.z, z, tol);
}

static KinChain chain(int n, bool planar) {
  KinChain C;
  std::memset(&C, 0, sizeof(C));
  C.n_dof = n;
  C.planar = planar ? 1 : 0;
  C.base_quat[0] = 1.0;
  for (int j = 0; j < kKinMaxDof; ++j) {
    C.joints[j].off_quat[0] = 1.0;
    C.joints[j].mount_quat[0] = 1.0;
  }
  return C;
}
static void set3(double* a, double x, double y, double z) { a[0] = x; a[1] = y; a[2] = z; }

int main() {
  const double hp = std::acos(-1.0) / 2.0;
  {  // ---- A
    KinChain C = chain(2, false);
    for (int j = 0; j < 2; ++j) set3(C.joints[j].axis, 0, 0, 1), set3(C.joints[j].axis_n, 0, 0, 1);
    set3(C.joints[0].off_pos, 1, 0, 0);
    set3(C.joints[1].off_pos, 0.5, 0, 0);
    // heap copies, so that the sanitizer sees every read of q / qd
    std::vector<double> q{hp, hp}, qd{1.0, 2.0};
    const KinFrameRef tip{KIN_LINK_END, 0, 1, 3u}, elbow{KIN_LINK_END, 0, 0, 1u}, base{KIN_BASE, 0, 0, 0u},
        j1{KIN_JOINT_END, 0, 1, 3u};
    auto nop = [](int, const KinFrame&) {};
    const KinFrame B = kin_walk<true>(C, base, q.data(), qd.data(), 1, nop);
    near3("A base pos", B.p, 0, 0, 0);
    near("A base quat", B.Q.w, 1.0);
    const KinFrame E = kin_walk<true>(C, elbow, q.data(), qd.data(), 1, nop);
    near3("A elbow pos", E.p, 0, 1, 0);
    near3("A elbow vel", E.v, -1, 0, 0);
    near3("A elbow w", E.w, 0, 0, 1);
    const KinFrame J1 = kin_walk<true>(C, j1, q.data(), qd.data(), 1, nop);
    near3("A joint-1 end pos", J1.p, 0, 1, 0);
    near3("A joint-1 end w", J1.w, 0, 0, 3);
    int visits = 0;
    const KinFrame T = kin_walk<true>(C, tip, q.data(), qd.data(), 1, [&](int, const KinFrame&) { ++visits; });
    near("A joints visited", visits, 2);
    near3("A tip pos", T.p, -0.5, 1, 0);
    near3("A tip vel", T.v, -1, -1.5, 0);
    near3("A tip w", T.w, 0, 0, 3);
    near("A tip quat w", T.Q.w, 0.0, 1e-15);
    near("A tip quat z", T.Q.z, 1.0, 1e-15);
    const m33 RT = rotmat(T.Q);
    const d3 WT = mul(RT, T.w);
    d3 Jqd_v = mk3(0, 0, 0), Jqd_w = mk3(0, 0, 0);
    kin_walk<true>(C, tip, q.data(), qd.data(), 1, [&](int j, const KinFrame& Ej) {
      const KinCol c = kin_column<true>(false, kin_ld3(C.joints[j].axis), Ej, T, RT, WT);
      if (j == 0) near3("A col0 v", c.v, 1, 0.5, 0), near3("A col0 w", c.w, 0, 0, 1);
      if (j == 1) near3("A col1 v", c.v, 0, 0.5, 0), near3("A col1 w", c.w, 0, 0, 1);
      // the rates of the columns: column 1 does not change in the tip's coordinates (the tip is rigid behind joint 1)
      if (j == 1) near3("A col1 vdot", c.vd, 0, 0, 0), near3("A col1 wdot", c.wd, 0, 0, 0);
      if (j == 0) near3("A col0 wdot", c.wd, 0, 0, 0);
      // column 0 in tip coordinates is (sin q1, 0.5 + cos q1, 0) [q1 = pi/2: (1, 0.5, 0)]: its rate is qd1 (cos q1, -sin q1, 0)
      if (j == 0) near3("A col0 vdot", c.vd, 0, -2, 0, 1e-15);
      Jqd_v = Jqd_v + qd[j] * c.v;
      Jqd_w = Jqd_w + qd[j] * c.w;
    });
    near3("A J qd = R^T v", Jqd_v, mulT(T.v, RT).x, mulT(T.v, RT).y, mulT(T.v, RT).z, 1e-15);
    near3("A J qd = w", Jqd_w, T.w.x, T.w.y, T.w.z);
    // the pose error of the tip against itself is zero, against a target 0.1 further along world y it is R^T (0, 0.1, 0)
    double e[6];
    kin_pose_error(T, T.p, T.Q, e);
    for (int i = 0; i < 6; ++i) near("A zero error", e[i], 0.0);
    kin_pose_error(T, T.p + mk3(0, 0.1, 0), d4{-T.Q.w, -T.Q.x, -T.Q.y, -T.Q.z}, e);  // -Q is the same rotation
    near("A e_v.y", e[1], -0.1, 1e-16);
    near("A e_w", std::fabs(e[3]) + std::fabs(e[4]) + std::fabs(e[5]), 0.0);
  }
  {  // ---- B
    KinChain C = chain(2, false);
    C.joints[0].prismatic = 1;
    set3(C.joints[0].axis, 0, 2, 0);
    set3(C.joints[0].axis_n, 0, 1, 0);
    set3(C.joints[1].axis, 1, 0, 0);
    set3(C.joints[1].axis_n, 1, 0, 0);
    set3(C.joints[0].off_pos, 0, 0, 1);
    set3(C.joints[1].off_pos, 0, 0, 1);
    std::vector<double> q{0.25, hp}, qd{3.0, 0.0};
    const KinFrameRef tip{KIN_LINK_END, 0, 1, 3u}, slider{KIN_JOINT_END, 0, 0, 1u};
    auto nop = [](int, const KinFrame&) {};
    const KinFrame S = kin_walk<true>(C, slider, q.data(), qd.data(), 1, nop);
    near3("B slider pos", S.p, 0, 0.5, 0);
    near3("B slider vel", S.v, 0, 6, 0);
    const KinFrame T = kin_walk<true>(C, tip, q.data(), qd.data(), 1, nop);
    near3("B tip pos", T.p, 0, -0.5, 1);
    near3("B tip vel", T.v, 0, 6, 0);
    const m33 RT = rotmat(T.Q);
    kin_walk<false>(C, tip, q.data(), nullptr, 1, [&](int j, const KinFrame& Ej) {
      const KinCol c = kin_column<false>(C.joints[j].prismatic != 0, kin_ld3(C.joints[j].axis), Ej, T, RT, mk3(0, 0, 0));
      if (j == 0) near3("B col0 v", c.v, 0, 0, -2), near3("B col0 w", c.w, 0, 0, 0);
      if (j == 1) near3("B col1 v", c.v, 0, -1, 0), near3("B col1 w", c.w, 1, 0, 0);
    });
    // a mount: the chain hung on a link (0, 0, 2) from the base moves every frame by it
    C.joints[0].branch_start = 1;
    set3(C.joints[0].mount_pos, 0, 0, 2);
    const KinFrameRef mount{KIN_MOUNT, 0, 0, 0u};
    near3("B mount", kin_walk<false>(C, mount, q.data(), nullptr, 1, nop).p, 0, 0, 2);
    near3("B tip on the mount", kin_walk<false>(C, tip, q.data(), nullptr, 1, nop).p, 0, -0.5, 3);
  }
  {  // ---- C
    KinChain C = chain(2, true);
    C.base_quat[0] = 1.0;
    C.base_quat[1] = 0.0;
    C.joints[0].off_pos[0] = 1.0;
    C.joints[1].off_pos[0] = 0.5;
    for (int j = 0; j < 2; ++j) C.joints[j].off_quat[0] = 1.0, C.joints[j].off_quat[1] = 0.0;
    std::vector<double> q{hp, hp}, qd{1.0, 2.0};
    const KinFrameRef tip{KIN_LINK_END, 0, 1, 3u};
    const KinFrame2 T = kin_walk2<true>(C, tip, q.data(), qd.data(), 1, [](int, const KinFrame2&) {});
    near("C tip x", T.p.x, -0.5, 2e-15);
    near("C tip y", T.p.y, 1.0, 2e-15);
    near("C tip vx", T.v.x, -1.0, 2e-15);
    near("C tip vy", T.v.y, -1.5, 2e-15);
    near("C tip w", T.w, 3.0);
    kin_walk2<true>(C, tip, q.data(), qd.data(), 1, [&](int j, const KinFrame2& Ej) {
      const KinCol2 c = kin_column2<true>(false, mk2(0, 0), Ej, T);
      near("C col w", c.w, 1.0);
      if (j == 0) near("C col0 vx", c.v.x, 1.0, 2e-15), near("C col0 vy", c.v.y, 0.5, 2e-15);
      if (j == 0) near("C col0 vdot x", c.vd.x, 0.0, 1e-15), near("C col0 vdot y", c.vd.y, -2.0, 1e-15);
      if (j == 1) near("C col1 vx", c.v.x, 0.0, 2e-15), near("C col1 vy", c.v.y, 0.5, 2e-15);
      if (j == 1) near("C col1 vdot", std::fabs(c.vd.x) + std::fabs(c.vd.y), 0.0, 1e-15);
    });
    C.joints[0].prismatic = 1;
    C.joints[0].axis[0] = 0.0;
    C.joints[0].axis[1] = 2.0;
    q[0] = 0.25;
    const KinFrameRef slider{KIN_JOINT_END, 0, 0, 1u};
    const KinFrame2 S = kin_walk2<true>(C, slider, q.data(), qd.data(), 1, [](int, const KinFrame2&) {});
    near("C slider y", S.p.y, 0.5);
    near("C slider vy", S.v.y, 2.0);
    const KinCol2 c = kin_column2<false>(true, kin_ld2(C.joints[0].axis), S, S);
    near("C slider col vy", c.v.y, 2.0);
    near("C slider col w", c.w, 0.0);
  }
  {  // ---- the 6 x 6 solve: A = diag(1..6) + u u^T, lower triangle packed
    double u[6] = {0.5, -0.25, 0.125, 1.0, -0.75, 0.3}, A[21], full[6][6], e[6] = {1, 2, 3, 4, 5, 6}, b[6];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) full[i][j] = u[i] * u[j] + (i == j ? i + 1.0 : 0.0);
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = full[i][j];
    std::memcpy(b, e, sizeof(b));
    if (!kin_cholesky6(A, e)) std::printf("FAIL cholesky refused a positive definite matrix\n"), ++g_fail;
    for (int i = 0; i < 6; ++i) {
      double r = -b[i];
      for (int j = 0; j < 6; ++j) r += full[i][j] * e[j];
      near("cholesky residual", r, 0.0, 1e-14);
    }
    A[0] = -1.0;
    std::memcpy(e, b, sizeof(b));
    if (kin_cholesky6(A, e)) std::printf("FAIL cholesky accepted a negative pivot\n"), ++g_fail;
    near("clamp low", kin_clamp(-2.0, -1.0, 1.0), -1.0);
    near("clamp high", kin_clamp(2.0, -1.0, 1.0), 1.0);
    near("clamp in", kin_clamp(0.5, -1.0, 1.0), 0.5);
  }
  if (g_fail) return 1;
  std::printf("kinematics host ok: frames, twists, columns and their rates, pose error, 6x6 solve\n");
  return 0;
}
