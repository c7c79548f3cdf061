// kinematics_smoke.cpp -- hip_direct_kin_map, hip_manip_kinematics_model and hip_pose_ik of include/rkh_adaptors.hpp compiled
// by g++ and linked against librkh.so (built like shortcut_smoke.cpp).  Prints one JSON line that
// tests/test_kinematics_smoke_gpu.py compares with the Python binding's answers for the same inputs.
// usage: kinematics_smoke <kinematics_scene.bin>
//   (scene, frame, point count, points as interleaved (q, qd) states, target pose, seed count, seeds, lower, upper)
#include <cstdio>
#include <vector>

#include "rkh_adaptors.hpp"

typedef std::vector<double> Point;

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

static void print_vec(const char* key, const double* v, std::size_t n, const char* tail) {
  std::printf("\"%s\": [", key);
  for (std::size_t i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", tail);
}

struct flat_matrix {  // the least a Matrix of the getters needs
  std::size_t cols;
  std::vector<double> a;
  double& operator()(std::size_t r, std::size_t c) { return a[r * cols + c]; }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0, n_points = 0, n_seeds = 0, frame = 0, n_dof = 0;
  rkh_chain_base base;
  rkh_pose target;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  bool ok = read_pod(f, &n_ops);
  ops.resize(n_ops);
  ok = ok && read_pod(f, ops.data(), n_ops) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(n_shapes);
  ok = ok && read_pod(f, shapes.data(), n_shapes) && read_pod(f, &n_dof) && read_pod(f, &frame) && read_pod(f, &n_points);
  const std::size_t n = std::size_t(n_dof);
  std::vector<double> states(ok ? std::size_t(n_points) * 2 * n : 0);
  ok = ok && read_pod(f, states.data(), states.size()) && read_pod(f, &target) && read_pod(f, &n_seeds);
  std::vector<double> seeds(ok ? std::size_t(n_seeds) * n : 0), lower(n), upper(n);
  ok = ok && read_pod(f, seeds.data(), seeds.size()) && read_pod(f, lower.data(), n) && read_pod(f, upper.data(), n);
  std::fclose(f);
  if (!ok) return 2;
  try {
    rkh::check(RKH_ABI_CHECK());
    auto ctx = rkh::make_context(0);
    auto scene = rkh::make_scene(ctx, ops.data(), n_ops, base, shapes.data(), n_shapes);
    std::vector<Point> pts;
    for (int32_t v = 0; v < n_points; ++v) pts.push_back(Point(states.begin() + v * 2 * n, states.begin() + (v + 1) * 2 * n));
    rkh::hip_direct_kin_map dk(scene, frame);
    const rkh::frame_pose_twist one = dk.map_to_space(pts[0], 0, 0);  // the two spaces only pick readers in the reference
    const std::vector<rkh::frame_pose_twist> all = dk.map_batch(pts);
    Point q0(n);
    for (std::size_t j = 0; j < n; ++j) q0[j] = pts[0][2 * j];
    const rkh::frame_pose_twist still = dk.map_to_space(q0);  // positions alone: zero rates
    rkh::hip_manip_kinematics_model model(scene, std::vector<int32_t>{frame, 0});
    model.apply_to_model(pts[0]);
    std::vector<double> J, Jd, J_only;
    model.getJacobianMatrixAndDerivative(J, Jd);
    model.getJacobianMatrix(J_only);
    flat_matrix M{n, std::vector<double>(model.getDependentVelocitiesCount() * n)};
    model.getJacobianMatrix(M);
    bool same = J_only == J && M.a == J;
    std::vector<Point> sd;
    for (int32_t s = 0; s < n_seeds; ++s) sd.push_back(Point(seeds.begin() + s * n, seeds.begin() + (s + 1) * n));
    const std::vector<Point> sol = rkh::hip_pose_ik(scene, frame, target, sd, lower, upper);
    bool threw = false;
    try {
      (void)dk.map_to_space(Point(n + 1));
    } catch (const std::range_error&) {
      threw = true;
    }
    std::printf("{");
    print_vec("pos", one.Position, 3, ", ");
    print_vec("quat", one.Quat, 4, ", ");
    print_vec("vel", one.Velocity, 3, ", ");
    print_vec("ang_vel", one.AngVelocity, 3, ", ");
    print_vec("last_pos", all.back().Position, 3, ", ");
    print_vec("last_vel", all.back().Velocity, 3, ", ");
    print_vec("still_pos", still.Position, 3, ", ");
    print_vec("still_vel", still.Velocity, 3, ", ");
    print_vec("jac", J.data(), J.size(), ", ");
    print_vec("jac_dot", Jd.data(), Jd.size(), ", ");
    std::printf("\"getters_agree\": %s, \"bad_point_throws\": %s, \"n_solutions\": %zu, ", same ? "true" : "false",
                threw ? "true" : "false", sol.size());
    print_vec("first_solution", sol.empty() ? nullptr : sol[0].data(), sol.empty() ? 0 : n, "}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "kinematics_smoke: %s\n", e.what());
    return 1;
  }
}
