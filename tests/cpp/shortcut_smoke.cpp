// shortcut_smoke.cpp -- manip_quasi_static_free_space::shortcut_path of include/rkh_adaptors.hpp compiled by g++ and
// linked against librkh.so (built like prm_paths_smoke.cpp): one path of points through the adaptor, with every hop tried
// and with hops of at most three points.  Prints one JSON line that tests/test_path_shortcut_gpu.py compares with the
// Python binding's answer for the same points.
// usage: shortcut_smoke <shortcut_scene.bin>   (scene, rkh_qs_space, point count, points)
#include <cstdio>
#include <vector>

#include "rkh_adaptors.hpp"

typedef std::vector<double> Point;

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

template <typename R>
static void print_result(const char* key, const R& r, const char* tail) {
  std::printf("\"%s\": {\"cost_in\": %.17g, \"cost_out\": %.17g, \"n_blocked\": %zu, \"keep\": [", key, r.cost_in, r.cost_out,
              r.n_blocked);
  for (std::size_t i = 0; i < r.keep.size(); ++i) std::printf("%s%zu", i ? ", " : "", r.keep[i]);
  std::printf("]}%s", tail);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0, n_points = 0;
  rkh_chain_base base;
  rkh_qs_space qs;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  bool ok = read_pod(f, &n_ops);
  ops.resize(n_ops);
  ok = ok && read_pod(f, ops.data(), n_ops) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(n_shapes);
  ok = ok && read_pod(f, shapes.data(), n_shapes) && read_pod(f, &qs) && read_pod(f, &n_points);
  const std::size_t n = std::size_t(qs.n_dof);
  std::vector<double> flat(ok ? std::size_t(n_points) * n : 0);
  ok = ok && read_pod(f, flat.data(), flat.size());
  std::fclose(f);
  if (!ok) return 2;
  try {
    rkh::check(RKH_ABI_CHECK());
    auto ctx = rkh::make_context(0);
    auto scene = rkh::make_scene(ctx, ops.data(), n_ops, base, shapes.data(), n_shapes);
    typedef rkh::manip_quasi_static_free_space<Point> QsSpace;
    QsSpace space(scene, qs);
    std::vector<Point> path;
    for (int32_t v = 0; v < n_points; ++v) path.push_back(Point(flat.begin() + v * n, flat.begin() + (v + 1) * n));
    const QsSpace::shortcut_result all = space.shortcut_path(path);
    const QsSpace::shortcut_result span3 = space.shortcut_path(path, 3);
    const QsSpace::shortcut_result one = space.shortcut_path(std::vector<Point>(1, path[0]));
    bool threw = false;
    try {
      (void)space.shortcut_path(std::vector<Point>());
    } catch (const std::runtime_error&) {
      threw = true;
    }
    std::printf("{");
    print_result("all", all, ", ");
    print_result("span3", span3, ", ");
    std::printf("\"single_point\": [");
    for (std::size_t i = 0; i < one.keep.size(); ++i) std::printf("%s%zu", i ? ", " : "", one.keep[i]);
    std::printf("], \"empty_path_throws\": %s}\n", threw ? "true" : "false");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shortcut_smoke: %s\n", e.what());
    return 1;
  }
}
