// arena_layout_test.cpp -- host-only check of planner_arena_layout (reak_amd/csrc/arena_layout.h): every range aligned,
// the ranges pairwise disjoint and inside the slab short of its guard tail, the total what the aligned sizes add up to,
// and the same answer twice.  Built with -fsanitize=address,undefined and run directly (tests/test_planner_arena_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "arena_layout.h"

using namespace rkh;

static int g_cases = 0;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "%s:%d: %s (case %d)\n", __FILE__, __LINE__, #cond, g_cases); \
      std::exit(1);                                                                  \
    }                                                                                \
  } while (0)

static void check_shape(uint32_t P, const std::vector<uint64_t>& max_vertices, bool mirror, bool profile, int D) {
  ++g_cases;
  // the planner's own rules: mirror planners of 64 problems and more cap a round at one query block of 128
  const uint32_t b_max = (mirror && P >= 64) ? 128u : 1024u;
  const int DP = D <= 4 ? 4 : (D <= 6 ? 6 : (D <= 8 ? 8 : (D <= 12 ? 12 : 16)));
  std::vector<uint64_t> capacity(P), sample_cap(P), mirror_bytes(P);
  for (uint32_t i = 0; i < P; ++i) {
    const uint64_t mv = max_vertices[i % max_vertices.size()];
    capacity[i] = planner_capacity_rows(mv);
    CHECK(capacity[i] % 256 == 0 && capacity[i] >= mv + 1 && capacity[i] < mv + 1 + 256);
    sample_cap[i] = planner_sample_cap(mv, b_max, 0);
    CHECK(sample_cap[i] >= (1u << 14) && sample_cap[i] >= 4 * (mv + 1) + 4 * b_max);
    mirror_bytes[i] = (capacity[i] + 31) / 32 * 1024;
  }
  ArenaShape s;
  s.P = P;
  s.capacity = capacity.data();
  s.sample_cap = sample_cap.data();
  s.mirror_bytes = mirror_bytes.data();
  s.b_max = b_max;
  s.probe_granule = 32;
  s.part_blocks = 7;
  s.prof_rounds = 8192;
  s.D = D;
  s.DP = DP;
  s.mirror = mirror;
  s.profile = profile;
  s.lane = D == 12;
  s.cand_bytes = size_t(644) * b_max + 256;
  s.lane_ws_bytes = size_t(P) * (2 * b_max + 32) * 1000 + 8;
  s.step_list_bytes = size_t(P) * (2 * b_max + 32) * 16;
  s.state_bytes = 80;
  s.prob_bytes = 112;
  s.nn_args_bytes = 168;
  s.edge_io_bytes = 152;
  s.init_bytes = 464;
  s.sample_seg_bytes = 40;
  s.goal_seg_bytes = 24;
  s.max_steps = 64;
  const ArenaLayout L = planner_arena_layout(s);

  std::vector<std::pair<size_t, size_t>> ranges;  // (offset, bytes) of everything handed out
  for (int r = 0; r < SR_COUNT; ++r) ranges.push_back({L.shared[r].off, L.shared[r].bytes});
  CHECK(L.problem.size() == size_t(P) * PR_COUNT);
  for (uint32_t i = 0; i < P; ++i)
    for (int r = 0; r < PR_COUNT; ++r) ranges.push_back({L.of(i, ProblemRange(r)).off, L.of(i, ProblemRange(r)).bytes});
  size_t sum = 0;
  for (const auto& r : ranges) {
    CHECK(r.first % kArenaAlign == 0);
    CHECK(r.first + r.second <= L.total - kArenaGuardBytes);
    sum += arena_align_up(r.second);
  }
  CHECK(L.total == sum + kArenaGuardBytes);
  for (size_t a = 0; a < ranges.size(); ++a)
    for (size_t b = a + 1; b < ranges.size(); ++b) {
      if (!ranges[a].second || !ranges[b].second) continue;
      CHECK(ranges[a].first + ranges[a].second <= ranges[b].first || ranges[b].first + ranges[b].second <= ranges[a].first);
    }
  // what the shape switches off takes no room, what it needs is there
  for (uint32_t i = 0; i < P; ++i) {
    CHECK((L.of(i, PR_MIRROR).bytes != 0) == mirror && (L.of(i, PR_CAND).bytes != 0) == mirror);
    CHECK((L.of(i, PR_ROUND_N).bytes != 0) == profile);
    CHECK(L.of(i, PR_TREE).bytes == capacity[i] * DP * 8 && L.of(i, PR_SAMPLES).bytes == sample_cap[i] * D * 8);
  }
  CHECK((L.shared[SR_LANE_WS].bytes != 0) == s.lane && (L.shared[SR_STEP_LIST1].bytes != 0) == s.lane);
  // the upload ranges are the leading ones
  for (int r = 0; r < SR_COUNT; ++r)
    CHECK((r < SR_UPLOAD_END) == (L.shared[r].off + L.shared[r].bytes <= L.upload_bytes && L.shared[r].off < L.upload_bytes));
  for (uint32_t i = 0; i < P; ++i) CHECK(L.of(i, PR_MT).off >= L.upload_bytes);
  // deterministic
  const ArenaLayout M = planner_arena_layout(s);
  CHECK(M.total == L.total && M.upload_bytes == L.upload_bytes && M.problem.size() == L.problem.size());
  for (int r = 0; r < SR_COUNT; ++r) CHECK(M.shared[r].off == L.shared[r].off && M.shared[r].bytes == L.shared[r].bytes);
  for (size_t k = 0; k < L.problem.size(); ++k) CHECK(M.problem[k].off == L.problem[k].off && M.problem[k].bytes == L.problem[k].bytes);
}

int main() {
  const std::vector<uint64_t> mixed = {1, 255, 256, 257, 2000};
  for (uint32_t P : {1u, 3u, 65u})
    for (int D : {3, 6, 12})
      for (int mirror = 0; mirror < 2; ++mirror)
        for (int profile = 0; profile < 2; ++profile) {
          check_shape(P, mixed, mirror != 0, profile != 0, D);
          check_shape(P, {300}, mirror != 0, profile != 0, D);
        }
  std::printf("arena layout ok: %d shapes\n", g_cases);
  return 0;
}
