// prox_records_depth_smoke.cpp -- the proximity socket of include/rkh_adaptors.hpp with its depth records switched on, on a
// scene with mesh shapes, compiled by g++ against librkh.so: hip_proxy_query_pair::findMinimumDistance() and
// gatherCollisionPoints answer from rkh_min_distance_records_depth / rkh_collision_records_depth, normals included; with
// the switch off (the default) the same socket still answers from the _meshes entries.  Prints one JSON line the calling
// test compares with the C-ABI's own answers (tests/test_depth_records_gpu.py).
// usage: prox_records_depth_smoke <scene.bin>
//   n_ops, ops, base, n_shapes, shapes, n_mesh_vertices, vertices [n][3], n_states, states [n_states][2 n_dof]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rkh_adaptors.hpp"

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

static void print3(const double* p) { std::printf("[%.17g, %.17g, %.17g]", p[0], p[1], p[2]); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0, n_verts = 0, n_states = 0;
  rkh_chain_base base;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  std::vector<double> verts;
  bool ok = read_pod(f, &n_ops);
  ops.resize(n_ops);
  ok = ok && read_pod(f, ops.data(), n_ops) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(n_shapes);
  ok = ok && read_pod(f, shapes.data(), n_shapes) && read_pod(f, &n_verts);
  verts.resize(3 * std::size_t(n_verts));
  ok = ok && read_pod(f, verts.data(), verts.size()) && read_pod(f, &n_states);
  if (!ok) return 2;
  try {
    rkh::check(RKH_ABI_CHECK());
    auto ctx = rkh::make_context(0);
    rkh_scene* raw = nullptr;
    rkh::check(rkh_scene_create_with_meshes(ctx.get(), ops.data(), n_ops, &base, shapes.data(), n_shapes, verts.data(),
                                            uint32_t(n_verts), &raw));
    std::shared_ptr<rkh_scene> scene(raw, [ctx](rkh_scene* p) { (void)rkh_scene_destroy(p); });
    const std::size_t D = 2 * std::size_t(rkh_scene_num_dof(scene.get()));
    std::vector<double> x(std::size_t(n_states) * D);
    if (!read_pod(f, x.data(), x.size())) return 2;
    std::fclose(f);
    rkh::hip_proxy_query_pair proxy(scene, true), plain(scene);
    if (!proxy.depth_records() || plain.depth_records()) return 3;
    std::printf("{\"states\": [");
    for (int32_t b = 0; b < n_states; ++b) {
      const std::vector<double> p(x.begin() + std::size_t(b) * D, x.begin() + std::size_t(b + 1) * D);
      proxy.apply_to_model(p);
      plain.apply_to_model(p);
      const auto finder = proxy.findMinimumDistance(), off = plain.findMinimumDistance();
      if (!finder || !off) return 3;
      if (off->normal()[0] != 0.0 || off->normal()[1] != 0.0 || off->normal()[2] != 0.0) return 5;  // default: no normal
      const rkh::proximity_record& r = finder->getLastResult();
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(r.mPoint1[k]) || !std::isfinite(r.mPoint2[k])) return 4;  // the distance-only fallback
      if (finder->getShape1Index() == rkh::hip_proximity_finder::no_shape) return 4;
      std::printf("%s{\"dist\": %.17g, \"p1\": ", b ? ", " : "", r.mDistance);
      print3(r.mPoint1);
      std::printf(", \"p2\": ");
      print3(r.mPoint2);
      std::printf(", \"n\": ");
      print3(finder->normal());
      std::printf(", \"plain_dist\": %.17g", off->getLastResult().mDistance);
      std::printf(", \"s1\": %u, \"s2\": %u, \"hits\": [", finder->getShape1Index(), finder->getShape2Index());
      std::vector<rkh::proximity_record> hits;
      std::vector<std::pair<uint32_t, uint32_t> > who;
      const bool any = proxy.gatherCollisionPoints(hits, &who);
      if (any != !hits.empty() || who.size() != hits.size()) return 3;
      for (std::size_t i = 0; i < hits.size(); ++i) {
        std::printf("%s{\"dist\": %.17g, \"p1\": ", i ? ", " : "", hits[i].mDistance);
        print3(hits[i].mPoint1);
        std::printf(", \"p2\": ");
        print3(hits[i].mPoint2);
        std::printf(", \"n\": ");
        print3(hits[i].mNormal);
        std::printf(", \"s1\": %u, \"s2\": %u}", who[i].first, who[i].second);
      }
      std::printf("]}");
    }
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
