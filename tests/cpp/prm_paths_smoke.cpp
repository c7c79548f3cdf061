// prm_paths_smoke.cpp -- hip_prm_planner::roadmap_solution() of include/rkh_adaptors.hpp compiled by g++ and linked
// against librkh.so (built like prox_records_smoke.cpp): PRM over a quasi-static scene through the adaptor and a
// point-to-point query object, then the start -> goal path through the finished roadmap.  Prints one JSON line that
// tests/test_roadmap_queries_gpu.py compares with the Python binding's answer for the same seed.
// usage: prm_paths_smoke <qs_scene.bin>   (scene, rkh_qs_space, rkh_rrt_params, sampling radius)
#include <cmath>
#include <cstdio>
#include <vector>

#include "rkh_adaptors.hpp"

typedef std::vector<double> Point;

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

struct P2PQuery {  // path_planning_p2p_query as far as the PRM adaptor uses it: nothing is ever registered
  Point start_pos, goal_pos;
  std::size_t max_num_results;
  std::size_t register_calls = 0;
  const Point& get_start_position() const { return start_pos; }
  const Point& get_goal_position() const { return goal_pos; }
  bool keep_going() const { return max_num_results > 0; }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0;
  rkh_chain_base base;
  rkh_qs_space qs;
  rkh_rrt_params qp;
  double sampling_radius = 1.0;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  bool ok = read_pod(f, &n_ops);
  ops.resize(n_ops);
  ok = ok && read_pod(f, ops.data(), n_ops) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(n_shapes);
  ok = ok && read_pod(f, shapes.data(), n_shapes) && read_pod(f, &qs) && read_pod(f, &qp) && read_pod(f, &sampling_radius);
  std::fclose(f);
  if (!ok) return 2;
  try {
    rkh::check(RKH_ABI_CHECK());
    auto ctx = rkh::make_context(0);
    auto scene = rkh::make_scene(ctx, ops.data(), n_ops, base, shapes.data(), n_shapes);
    typedef rkh::manip_quasi_static_free_space<Point> QsSpace;
    auto qspace = std::make_shared<QsSpace>(scene, qs);
    const std::size_t n = std::size_t(qs.n_dof);
    rkh::hip_prm_planner<QsSpace> pl(qspace, qp.max_vertices, 0, qp.steer_tol, qp.conn_tol, sampling_radius);
    bool threw = false;
    try {
      (void)pl.roadmap_solution();  // no roadmap yet
    } catch (const std::runtime_error&) {
      threw = true;
    }
    P2PQuery q{Point(qp.start, qp.start + n), Point(qp.goal, qp.goal + n), std::size_t(qp.max_results)};
    rkh::global_rng_seed(qp.seed);
    pl.solve_planning_query(q);
    const std::pair<std::vector<std::size_t>, double> sol = pl.roadmap_solution();
    const std::pair<std::vector<std::size_t>, double> again = pl.roadmap_solution();
    // the path runs over edges of motion_graph(); their weights, summed left to right, are the cost
    const rkh::hip_motion_graph<Point>& g = pl.motion_graph();
    double sum = 0.0;
    bool edges_ok = true;
    for (std::size_t i = 0; i + 1 < sol.first.size(); ++i) {
      double w = INFINITY;
      for (std::size_t e = 0; e < g.edges.size(); ++e) {
        const bool hit = (g.edges[e].first == sol.first[i] && g.edges[e].second == sol.first[i + 1]) ||
                         (g.edges[e].second == sol.first[i] && g.edges[e].first == sol.first[i + 1]);
        if (hit && g.edge_weight[e] < w) w = g.edge_weight[e];
      }
      edges_ok = edges_ok && std::isfinite(w);
      sum += w;
    }
    std::printf("{\"vertices\": %zu, \"edges\": %zu, \"cost\": %.17g, \"weight_sum\": %.17g, \"edges_ok\": %s, "
                "\"no_roadmap_throws\": %s, \"repeatable\": %s, \"register_calls\": %zu, \"path\": [",
                num_vertices(g), g.edges.size(), sol.second, sum, edges_ok ? "true" : "false", threw ? "true" : "false",
                (again == sol) ? "true" : "false", q.register_calls);
    for (std::size_t i = 0; i < sol.first.size(); ++i) std::printf("%s%zu", i ? ", " : "", sol.first[i]);
    std::printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "prm_paths_smoke: %s\n", e.what());
    return 1;
  }
}
