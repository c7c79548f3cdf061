// svp_walk_dir_host.cpp -- reak_amd/csrc/svp_walk_rules.h (with svp_device.h) read by a host compiler through the stand-in
// for <hip/hip_runtime.h> in tests/cpp/hip_host.  A program of its own: built with -fsanitize=address,undefined
// -ffp-contract=off and run by tests/test_svp_birrt_cpu.py, which compares what it prints, bit for bit, with the Python
// twins (tests/svp_ref.py::edge_walk forward, tests/svp_back_ref.py::edge_walk_back backward).
//
// It walks every row it reads in both directions the way svp_walk_dir.hip's three kernels do -- solve (count, first time),
// passes of 32 points (point j of a pass at the row's next time moved j steps, the next pass 32 steps on), scan (bounds only:
// no scene here), finish -- and prints the tested times pass by pass, the counts and the returned point as hex floats.
//
// stdin:  n min_interval / n lines "lower upper speed accel" / B / B lines "a[2n] b[2n] fraction", all numbers %la
// stdout: per row and direction  "walk <row> <back> T <T> K <K>", "pass <p> <times...>", "out <nc> <reached> <x[2n]>"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../reak_amd/csrc/svp_walk_rules.h"

using namespace rkh;

static int g_fail = 0;
static void truth(const char* what, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++g_fail;
  }
}

static void walk_row(const SvpDev& sp, int row, bool back, const double* a, const double* b, double fraction) {
  const int D = 2 * sp.n;
  std::vector<double> peak(sp.n), out(D), last(D), x(D);
  const double T = svp_reach(sp, a, b, peak.data());
  const double* origin = svp_walk_origin(back) == kSvpWalkEndA ? a : b;
  uint32_t nc = 0;
  int reached = 0;
  bool over = false;
  uint32_t K = 0;
  double dt = 0.0;
  if (T < INFINITY) {
    dt = svp_walk_dt(back, T, fraction);
    K = svp_walk_count(back, sp.min_interval, T, dt, kSvpWalkMaxPoints, &over);
  }
  std::printf("walk %d %d T %a K %u\n", row, int(back), T, K);
  if (!(T < INFINITY) || over) {
    std::printf("out 0 0");
    for (int c = 0; c < D; ++c) std::printf(" %a", origin[c]);
    std::printf("\n");
    return;
  }
  for (int c = 0; c < D; ++c) last[c] = origin[c];
  double d_next = svp_walk_first(back, sp.min_interval, T);
  uint32_t k = 0;
  bool failed = false;
  for (uint32_t pass = 0; k < K && !failed; ++pass) {
    std::printf("pass %u", pass);
    uint32_t j = 0;
    for (; j < kSvpWalkPass && k + j < K; ++j) {
      const double d = svp_walk_advance(back, d_next, sp.min_interval, j);
      truth("a tested time is one of the loop's", svp_walk_open(back, d, dt));
      std::printf(" %a", d);
      svp_point(sp, a, b, peak.data(), T, d, x.data(), nullptr);
      ++nc;
      if (!svp_in_bounds(sp, x.data())) {
        failed = true;
        break;
      }
      last = x;
    }
    std::printf("\n");
    k += j;
    d_next = svp_walk_advance(back, d_next, sp.min_interval, kSvpWalkPass);
  }
  if (failed) {
    out = last;
  } else {
    reached = 1;
    const SvpWalkEnd end = svp_walk_result(back, fraction);
    if (end == kSvpWalkEndPoint) svp_point(sp, a, b, peak.data(), T, dt, out.data(), nullptr);
    else
      for (int c = 0; c < D; ++c) out[c] = (end == kSvpWalkEndA ? a : b)[c];
  }
  std::printf("out %u %d", nc, reached);
  for (int c = 0; c < D; ++c) std::printf(" %a", out[c]);
  std::printf("\n");
}

int main() {
  // the rules by hand: min_interval 0.25, T 1 -- forward 0.25, 0.5, 0.75 below dt = 1 (strict: 1.0 itself is not tested);
  // backward 0.75, 0.5, 0.25 above dt = 0; T below min_interval: nothing either way
  bool over = true;
  truth("forward count", svp_walk_count(false, 0.25, 1.0, svp_walk_dt(false, 1.0, 1.0), 100, &over) == 3 && !over);
  truth("backward count", svp_walk_count(true, 0.25, 1.0, svp_walk_dt(true, 1.0, 1.0), 100, &over) == 3 && !over);
  truth("backward half", svp_walk_count(true, 0.25, 1.0, svp_walk_dt(true, 1.0, 0.5), 100, &over) == 1 && !over);
  truth("forward half", svp_walk_count(false, 0.25, 1.0, svp_walk_dt(false, 1.0, 0.5), 100, &over) == 1 && !over);
  truth("short forward", svp_walk_count(false, 0.25, 0.2, 0.2, 100, &over) == 0 && !over);
  truth("short backward", svp_walk_count(true, 0.25, 0.2, 0.0, 100, &over) == 0 && !over);
  truth("cap forward", svp_walk_count(false, 0.25, 1.0, 1.0, 2, &over) == 2 && over);
  truth("cap backward", svp_walk_count(true, 0.25, 1.0, 0.0, 2, &over) == 2 && over);
  truth("first", svp_walk_first(false, 0.25, 1.0) == 0.25 && svp_walk_first(true, 0.25, 1.0) == 0.75);
  truth("advance", svp_walk_advance(false, 0.25, 0.25, 2) == 0.75 && svp_walk_advance(true, 0.75, 0.25, 2) == 0.25);
  truth("origin", svp_walk_origin(false) == kSvpWalkEndA && svp_walk_origin(true) == kSvpWalkEndB);
  truth("result 1", svp_walk_result(false, 1.0) == kSvpWalkEndB && svp_walk_result(true, 1.0) == kSvpWalkEndA);
  truth("result 0", svp_walk_result(false, 0.0) == kSvpWalkEndA && svp_walk_result(true, 0.0) == kSvpWalkEndB);
  truth("result between", svp_walk_result(false, 0.5) == kSvpWalkEndPoint && svp_walk_result(true, 0.5) == kSvpWalkEndPoint);

  SvpDev sp;
  std::memset(&sp, 0, sizeof(sp));
  int n = 0;
  if (std::scanf("%d %la", &n, &sp.min_interval) != 2 || n < 1 || n > kSvpMaxDof) return 2;
  sp.n = n;
  for (int i = 0; i < kSvpMaxDof; ++i) sp.speed[i] = sp.accel[i] = sp.vm[i] = 1.0;
  for (int i = 0; i < n; ++i) {
    if (std::scanf("%la %la %la %la", &sp.lower[i], &sp.upper[i], &sp.speed[i], &sp.accel[i]) != 4) return 2;
    sp.vm[i] = sp.speed[i] / sp.accel[i];
  }
  int B = 0;
  if (std::scanf("%d", &B) != 1 || B < 0) return 2;
  const int D = 2 * n;
  std::vector<double> a(D), b(D);
  for (int e = 0; e < B; ++e) {
    double f = 0.0;
    for (int c = 0; c < D; ++c)
      if (std::scanf("%la", &a[c]) != 1) return 2;
    for (int c = 0; c < D; ++c)
      if (std::scanf("%la", &b[c]) != 1) return 2;
    if (std::scanf("%la", &f) != 1) return 2;
    walk_row(sp, e, false, a.data(), b.data(), f);
    walk_row(sp, e, true, a.data(), b.data(), f);
  }
  if (g_fail) return 1;
  std::printf("svp walk dir host ok: %d rows in both directions\n", B);
  return 0;
}
