// svp_rrt_smoke.cpp -- the rkh_svp_rrt_* entries of include/rkh.h called from a C++ program compiled by g++ and linked
// against librkh.so (built like svp_smoke.cpp), after the ABI handshake.  Prints one JSON line that
// tests/test_svp_rrt_smoke_gpu.py compares with the Python binding's answers for the same problems.
// usage: svp_rrt_smoke <svp_rrt_scene.bin>
//   (scene, the rkh_svp_space as bytes, problem count P, rkh_svp_rrt_params [P] as bytes)
#include <cstdio>
#include <vector>

#include "rkh.h"

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

static void print_vec(const char* key, const double* v, std::size_t n, const char* tail) {
  std::printf("\"%s\": [", key);
  for (std::size_t i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", tail);
}

template <typename I>
static void print_ints(const char* key, const I* v, std::size_t n, const char* tail) {
  std::printf("\"%s\": [", key);
  for (std::size_t i = 0; i < n; ++i) std::printf("%s%lu", i ? ", " : "", static_cast<unsigned long>(v[i]));
  std::printf("]%s", tail);
}

#define CHECK(expr)                                                                  \
  do {                                                                               \
    if ((expr) != RKH_OK) {                                                          \
      std::fprintf(stderr, "svp_rrt_smoke: %s: %s\n", #expr, rkh_last_error());      \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0, P = 0;
  rkh_chain_base base;
  rkh_svp_space space;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  bool ok = read_pod(f, &n_ops);
  ops.resize(ok ? n_ops : 0);
  ok = ok && read_pod(f, ops.data(), ops.size()) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(ok ? n_shapes : 0);
  ok = ok && read_pod(f, shapes.data(), shapes.size()) && read_pod(f, &space) && read_pod(f, &P);
  std::vector<rkh_svp_rrt_params> params(ok && P > 0 ? std::size_t(P) : 0);
  ok = ok && read_pod(f, params.data(), params.size());
  std::fclose(f);
  if (!ok || params.empty() || space.struct_size != sizeof(rkh_svp_space) || params[0].struct_size != sizeof(rkh_svp_rrt_params))
    return 2;
  const std::size_t D = 2 * std::size_t(space.n_dof), np = params.size();
  CHECK(RKH_ABI_CHECK());
  rkh_ctx* ctx = nullptr;
  rkh_scene* scene = nullptr;
  rkh_svp_rrt* planner = nullptr;
  CHECK(rkh_ctx_create(0, &ctx));
  CHECK(rkh_scene_create(ctx, ops.data(), n_ops, &base, shapes.data(), n_shapes, &scene));
  // a struct of another size is refused and leaves nothing behind
  std::vector<rkh_svp_rrt_params> wrong(params);
  wrong[np - 1].struct_size -= 8;
  const bool refused = rkh_svp_rrt_create_batch(scene, &space, wrong.data(), uint32_t(np), &planner) == RKH_ERR_BAD_ARG && !planner;
  CHECK(rkh_svp_rrt_create_batch(scene, &space, params.data(), uint32_t(np), &planner));
  rkh_svp_rrt_stats first, stats;
  CHECK(rkh_svp_rrt_solve(planner, 2, &first));   // two rounds, then the rest
  CHECK(rkh_svp_rrt_solve(planner, -1, &stats));
  std::vector<uint32_t> n_vertices(np), iterations(np), goal_parent(np);
  CHECK(rkh_svp_rrt_get_status(planner, n_vertices.data(), iterations.data(), goal_parent.data()));
  std::printf("{");
  print_ints("n_vertices", n_vertices.data(), np, ", ");
  print_ints("iterations", iterations.data(), np, ", ");
  print_ints("goal_parent", goal_parent.data(), np, ", ");
  for (std::size_t i = 0; i < np; ++i) {
    const uint32_t cap = params[i].max_vertices;
    std::vector<double> verts(cap * D), et(cap), pts((std::size_t(cap) + 1) * D);
    std::vector<uint32_t> parent(cap);
    uint32_t V = 0, n_points = 0;
    double duration = 0.0;
    CHECK(rkh_svp_rrt_get_tree(planner, uint32_t(i), verts.data(), parent.data(), et.data(), cap, &V));
    CHECK(rkh_svp_rrt_get_solution(planner, uint32_t(i), pts.data(), cap + 1, &n_points, &duration));
    char key[32];
    std::snprintf(key, sizeof(key), "vertices_%zu", i);
    print_vec(key, verts.data(), V * D, ", ");
    std::snprintf(key, sizeof(key), "parent_%zu", i);
    print_ints(key, parent.data(), V, ", ");
    std::snprintf(key, sizeof(key), "edge_time_%zu", i);
    print_vec(key, et.data(), V, ", ");
    std::snprintf(key, sizeof(key), "solution_%zu", i);
    print_vec(key, pts.data(), n_points * D, ", ");
    std::printf("\"duration_%zu\": %.17g, ", i, duration);
  }
  std::printf("\"first_rounds\": %lu, \"rounds\": %lu, \"finished\": %lu, \"total_iterations\": %lu, \"total_vertices\": %lu, ",
              static_cast<unsigned long>(first.rounds), static_cast<unsigned long>(stats.rounds),
              static_cast<unsigned long>(stats.problems_finished), static_cast<unsigned long>(stats.iterations),
              static_cast<unsigned long>(stats.vertices));
  std::printf("\"wrong_size_refused\": %s}\n", refused ? "true" : "false");
  rkh_svp_rrt_destroy(planner);
  rkh_scene_destroy(scene);
  rkh_ctx_destroy(ctx);
  return 0;
}
