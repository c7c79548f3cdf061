// round_carry_test.cpp -- host-only check of the round-carry rule (reak_amd/csrc/round_carry.h) at its edges, and of the
// stash ranges it adds to the planner's arena (reak_amd/csrc/arena_layout.h).  Built with -fsanitize=address,undefined
// and run directly (tests/test_round_carry_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "arena_layout.h"
#include "round_carry.h"

using namespace rkh;

static int g_checks = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// One round boundary played through the header, the way commit_kernel and carry_restore_kernel use it: the old round's
// nn_idx [B_old] and `cut`, the new round's nn_idx [B_new]; returns the reuse mark of every new slot.  The stash is
// allocated at exactly `carried` entries, so a read past it is an AddressSanitizer error.
static std::vector<int> play(const std::vector<uint32_t>& nn_old, uint32_t cut, bool valid, const std::vector<uint32_t>& nn_new,
                             uint32_t* carried_out = nullptr) {
  const uint32_t B_old = uint32_t(nn_old.size()), B_new = uint32_t(nn_new.size());
  const uint32_t carried = carry_count(B_old, cut, valid);
  std::vector<uint32_t> stash(carried);
  for (uint32_t j = 0; j < carried; ++j) stash[j] = nn_old[carry_old_slot(j, cut)];
  std::vector<int> mark(B_new);
  for (uint32_t b = 0; b < B_new; ++b) mark[b] = carry_reuses(b, carried, B_new, nn_new[b], stash.data()) ? 1 : 0;
  if (carried_out) *carried_out = carried;
  return mark;
}

static uint32_t count(const std::vector<int>& m) {
  uint32_t n = 0;
  for (int v : m) n += uint32_t(v);
  return n;
}

static void rule_tests() {
  // the slot mapping and the carried count
  CHECK(carry_old_slot(0, 0) == 0 && carry_old_slot(0, 5) == 5 && carry_old_slot(7, 5) == 12);
  CHECK(carry_count(10, 10, true) == 0);  // cut = B: nothing discarded
  CHECK(carry_count(10, 1, true) == 9);   // cut = 1
  CHECK(carry_count(10, 0, true) == 10);  // the first candidate was invalid already
  CHECK(carry_count(0, 0, true) == 0);
  CHECK(carry_count(10, 3, false) == 0);  // create, feature off, problem done
  CHECK(carry_count(4096, 1, true) == 4095 && carry_count(4096, 0, true) == 4096);  // b_max
  // clipped to the new B
  CHECK(carry_usable(9, 4) == 4 && carry_usable(9, 9) == 9 && carry_usable(9, 20) == 9 && carry_usable(0, 20) == 0 &&
        carry_usable(9, 0) == 0);
  CHECK(carry_expected_reuse(0, 100) == 0 && carry_expected_reuse(8, 100) == 7 && carry_expected_reuse(16, 8) == 7 &&
        carry_expected_reuse(100, 0) == 0);
  CHECK(carry_expected_reuse(4096, 4096) <= 4096);

  std::vector<uint32_t> old_nn(12);
  for (uint32_t b = 0; b < 12; ++b) old_nn[b] = 100 + b;
  uint32_t carried = 99;
  // carried = 0: nothing is reused whatever the indices say
  CHECK(count(play(old_nn, 12, true, old_nn, &carried)) == 0 && carried == 0);
  CHECK(count(play(old_nn, 3, false, {103, 104, 105}, &carried)) == 0 && carried == 0);
  CHECK(count(play({}, 0, true, {1, 2, 3}, &carried)) == 0 && carried == 0);
  // cut = 1, every index unchanged, new B larger than carried: the 11 carried slots reuse, the rest do not
  {
    std::vector<uint32_t> nw(20, 7u);
    for (uint32_t b = 0; b < 11; ++b) nw[b] = old_nn[b + 1];
    const std::vector<int> m = play(old_nn, 1, true, nw, &carried);
    CHECK(carried == 11 && count(m) == 11);
    for (uint32_t b = 0; b < 20; ++b) CHECK(m[b] == (b < 11 ? 1 : 0));
  }
  // a slot beyond the carried ones does not reuse even if its index happens to equal a stale value
  {
    std::vector<uint32_t> nw = {104, 105, 106, 107, 108, 109, 110, 111, 111, 111};
    const std::vector<int> m = play(old_nn, 4, true, nw, &carried);
    CHECK(carried == 8 && count(m) == 8 && m[8] == 0 && m[9] == 0);
  }
  // new B equal to carried / smaller than carried (the surplus is dropped: no slot at or beyond B_new exists)
  {
    std::vector<uint32_t> nw = {104, 105, 106, 107, 108, 109, 110, 111};
    CHECK(count(play(old_nn, 4, true, nw, &carried)) == 8 && carried == 8);
    nw.resize(3);
    CHECK(count(play(old_nn, 4, true, nw, &carried)) == 3 && carried == 8);
    nw.clear();
    CHECK(count(play(old_nn, 4, true, nw)) == 0);
  }
  // a changed index at slot 0, in the middle and at the last carried slot: exactly that slot is steered again
  for (uint32_t changed : {0u, 4u, 7u}) {
    std::vector<uint32_t> nw = {104, 105, 106, 107, 108, 109, 110, 111, 5, 5};
    nw[changed] = 1000;  // a vertex the round before added
    const std::vector<int> m = play(old_nn, 4, true, nw);
    for (uint32_t b = 0; b < 10; ++b) CHECK(m[b] == ((b < 8 && b != changed) ? 1 : 0));
  }
  // b_max candidates, cut = 1: the mapping reaches the last old slot and no further
  {
    std::vector<uint32_t> big(4096), nw(4096);
    for (uint32_t b = 0; b < 4096; ++b) big[b] = b * 3u;
    for (uint32_t b = 0; b < 4095; ++b) nw[b] = big[b + 1];
    nw[4095] = big[4095];
    const std::vector<int> m = play(big, 1, true, nw, &carried);
    CHECK(carried == 4095 && count(m) == 4095 && m[4094] == 1 && m[4095] == 0);
  }
  // which rounds carry: the step-wise gate and the minimum, one function for both readers
  CHECK(!carry_round(50000, 0, 0xFFFFFFFFu, kCarryOff));
  CHECK(carry_round(0, 0, 0xFFFFFFFFu, 0) && carry_round(5, 5, 6, 5) && !carry_round(6, 5, 6, 5) && !carry_round(4, 5, 6, 0));
  CHECK(!carry_round(99, 10, 0xFFFFFFFFu, 100) && carry_round(100, 10, 0xFFFFFFFFu, 100) && !carry_round(100, 101, 0xFFFFFFFFu, 100));
}

// the arena layout's invariants (tests/cpp/arena_layout_test.cpp) with the stash ranges in it
static void layout_tests() {
  for (uint32_t P : {1u, 3u, 65u})
    for (int lane = 0; lane < 2; ++lane)
      for (int carry = 0; carry < 2; ++carry) {
        const uint32_t b_max = P >= 64 ? 128u : 1024u;
        const int D = 12, DP = 12;
        std::vector<uint64_t> capacity(P), sample_cap(P), mirror_bytes(P);
        for (uint32_t i = 0; i < P; ++i) {
          capacity[i] = planner_capacity_rows(300 + 7 * i);
          sample_cap[i] = planner_sample_cap(300 + 7 * i, b_max, 0);
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
        s.mirror = true;
        s.lane = lane != 0;
        s.carry = carry != 0;
        s.cand_bytes = size_t(644) * b_max + 256;
        s.lane_ws_bytes = size_t(P) * (2 * b_max + 32) * 1000 + 8;
        s.step_list_bytes = size_t(P) * (2 * b_max + 32) * 16;
        s.state_bytes = 96;
        s.prob_bytes = 152;
        s.nn_args_bytes = 168;
        s.edge_io_bytes = 152;
        s.init_bytes = 464;
        s.sample_seg_bytes = 40;
        s.goal_seg_bytes = 24;
        s.max_steps = 64;
        const ArenaLayout L = planner_arena_layout(s);
        std::vector<std::pair<size_t, size_t>> ranges;
        for (int r = 0; r < SR_COUNT; ++r) ranges.push_back({L.shared[r].off, L.shared[r].bytes});
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
        const bool on = lane && carry;  // the reuse needs the step-wise launches of the two-lanes mapping
        for (uint32_t i = 0; i < P; ++i) {
          CHECK(L.of(i, PR_STASH_X).bytes == (on ? size_t(b_max) * D * 8 : 0));
          CHECK(L.of(i, PR_STASH_NN).bytes == (on ? size_t(b_max) * 4 : 0));
          CHECK(L.of(i, PR_STASH_STEPS).bytes == (on ? size_t(b_max) * 4 : 0));
          CHECK(L.of(i, PR_STASH_ACCEPT).bytes == (on ? size_t(b_max) : 0));
          // the stash mirrors the round's own buffers
          CHECK(!on || (L.of(i, PR_STASH_X).bytes == L.of(i, PR_X_OUT).bytes && L.of(i, PR_STASH_NN).bytes == L.of(i, PR_NN_IDX).bytes &&
                        L.of(i, PR_STASH_STEPS).bytes == L.of(i, PR_STEPS).bytes && L.of(i, PR_STASH_ACCEPT).bytes == L.of(i, PR_ACCEPT).bytes));
          CHECK(L.of(i, PR_MT).off >= L.upload_bytes);
        }
        if (!on) {  // switched off, the slab is what it was without the feature
          ArenaShape t = s;
          t.carry = false;
          CHECK(planner_arena_layout(t).total == L.total);
        }
      }
}

int main() {
  rule_tests();
  layout_tests();
  std::printf("round carry ok: %d checks\n", g_checks);
  return 0;
}
