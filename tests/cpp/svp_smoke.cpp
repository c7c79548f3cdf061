// svp_smoke.cpp -- the rkh_svp_* entries of include/rkh.h called from a C++ program compiled by g++ and linked against
// librkh.so (built like kinematics_smoke.cpp), after the ABI handshake.  Prints one JSON line that
// tests/test_svp_smoke_gpu.py compares with the Python binding's answers for the same inputs.
// usage: svp_smoke <svp_scene.bin>
//   (scene, the rkh_svp_space as bytes, pair count B, a [B][2n], b [B][2n], fraction [B])
#include <cstdio>
#include <vector>

#include "rkh.h"

template <typename T>
static bool read_pod(FILE* f, T* out, std::size_t n = 1) {
  return std::fread(out, sizeof(T), n, f) == n;
}

static void print_vec(const char* key, const double* v, std::size_t n, const char* tail) {
  std::printf("\"%s\": [", key);
  for (std::size_t i = 0; i < n; ++i) {
    if (v[i] != v[i] || v[i] - v[i] != 0.0) std::printf("%s\"%s\"", i ? ", " : "", v[i] > 0 ? "inf" : (v[i] < 0 ? "-inf" : "nan"));
    else std::printf("%s%.17g", i ? ", " : "", v[i]);
  }
  std::printf("]%s", tail);
}

template <typename I>
static void print_ints(const char* key, const I* v, std::size_t n, const char* tail) {
  std::printf("\"%s\": [", key);
  for (std::size_t i = 0; i < n; ++i) std::printf("%s%lu", i ? ", " : "", static_cast<unsigned long>(v[i]));
  std::printf("]%s", tail);
}

#define CHECK(expr)                                                              \
  do {                                                                           \
    if ((expr) != RKH_OK) {                                                      \
      std::fprintf(stderr, "svp_smoke: %s: %s\n", #expr, rkh_last_error());      \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_ops = 0, n_shapes = 0, B = 0;
  rkh_chain_base base;
  rkh_svp_space space;
  std::vector<rkh_kte_op> ops;
  std::vector<rkh_shape> shapes;
  bool ok = read_pod(f, &n_ops);
  ops.resize(ok ? n_ops : 0);
  ok = ok && read_pod(f, ops.data(), ops.size()) && read_pod(f, &base) && read_pod(f, &n_shapes);
  shapes.resize(ok ? n_shapes : 0);
  ok = ok && read_pod(f, shapes.data(), shapes.size()) && read_pod(f, &space) && read_pod(f, &B);
  const std::size_t D = ok ? 2 * std::size_t(space.n_dof) : 0, n = D / 2, nb = ok ? std::size_t(B) : 0;
  std::vector<double> a(nb * D), b(nb * D), fraction(nb);
  ok = ok && read_pod(f, a.data(), a.size()) && read_pod(f, b.data(), b.size()) && read_pod(f, fraction.data(), nb);
  std::fclose(f);
  if (!ok || space.struct_size != sizeof(rkh_svp_space)) return 2;
  CHECK(RKH_ABI_CHECK());
  rkh_ctx* ctx = nullptr;
  rkh_scene* scene = nullptr;
  CHECK(rkh_ctx_create(0, &ctx));
  CHECK(rkh_scene_create(ctx, ops.data(), n_ops, &base, shapes.data(), n_shapes, &scene));
  std::vector<uint8_t> inb(nb), reached(nb);
  std::vector<double> time(nb), peak(nb * n), out(nb * D), walk_time(nb), kdist(3 * 4), t(nb * 3), traj(nb * 3 * D);
  std::vector<uint32_t> n_checked(nb), kidx(3 * 4);
  const uint32_t Bu = uint32_t(B);
  CHECK(rkh_svp_in_bounds(&space, a.data(), Bu, inb.data()));
  CHECK(rkh_svp_reach_time(ctx, &space, a.data(), b.data(), Bu, time.data(), peak.data()));
  CHECK(rkh_svp_nearest(ctx, &space, a.data(), Bu, b.data(), 3, 4, 0, kidx.data(), kdist.data()));
  CHECK(rkh_svp_edge_check(scene, &space, a.data(), b.data(), Bu, fraction.data(), out.data(), walk_time.data(), n_checked.data(),
                           reached.data()));
  for (std::size_t e = 0; e < nb; ++e)
    for (int m = 0; m < 3; ++m) t[e * 3 + m] = (time[e] - time[e] == 0.0 ? time[e] : 1.0) * (0.25 + 0.25 * m);
  CHECK(rkh_svp_interpolate(ctx, &space, a.data(), b.data(), Bu, t.data(), 3, traj.data(), nullptr));
  space.struct_size -= 8;  // another header's struct: refused, not read past
  const bool refused = rkh_svp_reach_time(ctx, &space, a.data(), b.data(), Bu, time.data(), nullptr) == RKH_ERR_BAD_ARG;
  std::printf("{");
  print_ints("in_bounds", inb.data(), nb, ", ");
  print_vec("time", time.data(), nb, ", ");
  print_vec("peak", peak.data(), peak.size(), ", ");
  print_ints("knn_idx", kidx.data(), kidx.size(), ", ");
  print_vec("knn_dist", kdist.data(), kdist.size(), ", ");
  print_vec("out", out.data(), out.size(), ", ");
  print_vec("walk_time", walk_time.data(), nb, ", ");
  print_ints("n_checked", n_checked.data(), nb, ", ");
  print_ints("reached", reached.data(), nb, ", ");
  print_vec("traj", traj.data(), traj.size(), ", ");
  std::printf("\"wrong_size_refused\": %s}\n", refused ? "true" : "false");
  rkh_scene_destroy(scene);
  rkh_ctx_destroy(ctx);
  return 0;
}
