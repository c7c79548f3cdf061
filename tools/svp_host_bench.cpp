// svp_host_bench.cpp -- reak_amd/csrc/svp_device.h on one host core, for tools/measure_svp_space.py: reach times of N
// seeded pairs of a 6-joint space, then the interpolated points of their walks with the bounds rule (no collision test: the
// host has none).  Prints one JSON line.   usage: svp_host_bench <pairs> <min_interval>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../reak_amd/csrc/svp_device.h"

using namespace rkh;

static unsigned long long g_state = 1ull;
static double uni() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return double(g_state >> 11) / 9007199254740992.0;
}

int main(int argc, char** argv) {
  const size_t N = argc > 1 ? size_t(std::atol(argv[1])) : 1000000;
  SvpDev sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.n = 6;
  sp.min_interval = argc > 2 ? std::atof(argv[2]) : 0.05;
  for (int i = 0; i < 6; ++i) sp.speed[i] = sp.accel[i] = sp.vm[i] = 1.0, sp.lower[i] = -2.0, sp.upper[i] = 2.0;
  std::vector<double> a(N * 12), b(N * 12), T(N), peak(N * 6);
  for (size_t i = 0; i < N * 12; ++i) a[i] = (i & 1) ? 2 * uni() - 1 : 4 * uni() - 2, b[i] = (i & 1) ? 2 * uni() - 1 : 4 * uni() - 2;
  auto t0 = std::chrono::steady_clock::now();
  size_t finite = 0;
  for (size_t e = 0; e < N; ++e) finite += (T[e] = svp_reach(sp, &a[e * 12], &b[e * 12], &peak[e * 6])) < INFINITY;
  auto t1 = std::chrono::steady_clock::now();
  size_t points = 0, inside = 0;
  double x[12], sink = 0.0;
  const size_t walks = N < 20000 ? N : 20000;
  for (size_t e = 0; e < walks; ++e) {
    if (!(T[e] < INFINITY)) continue;
    for (double d = sp.min_interval; d < T[e]; d += sp.min_interval) {
      svp_point(sp, &a[e * 12], &b[e * 12], &peak[e * 6], T[e], d, x, nullptr);
      inside += svp_in_bounds(sp, x);
      sink += x[0];
      ++points;
    }
  }
  auto t2 = std::chrono::steady_clock::now();
  const double s_reach = std::chrono::duration<double>(t1 - t0).count(), s_walk = std::chrono::duration<double>(t2 - t1).count();
  std::printf("{\"pairs\": %zu, \"finite\": %zu, \"reach_s\": %.6f, \"pairs_per_s\": %.1f, \"walks\": %zu, \"walk_points\": %zu, "
              "\"walk_s\": %.6f, \"points_per_s\": %.1f, \"inside\": %zu, \"sink\": %.3f}\n",
              N, finite, s_reach, N / s_reach, walks, points, s_walk, points / s_walk, inside, sink);
  return 0;
}
