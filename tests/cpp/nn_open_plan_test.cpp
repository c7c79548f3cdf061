// The open rule and the work-item arithmetic of the mirror sweep's second pass (reak_amd/csrc/nn_mirror.h), pinned at
// their edges on the host: built with AddressSanitizer and UBSan by tests/test_nn_open_plan_cpu.py and run directly.
// The header's plan section uses no HIP: a host compiler reads it as it is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "nn_mirror.h"

using namespace rkh;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

// Replays what the blocks of one row slice do with a list of `listed` entries on a grid of `grid_blocks` blocks per
// slice: every entry must be taken by exactly one live slot, every pad slot must read an entry inside the block's own
// range, and no slot may read past the list.
static void replay(uint32_t listed, uint32_t grid_blocks) {
  std::vector<uint32_t> taken(listed, 0u);
  uint32_t working = 0;
  for (uint32_t by = 0; by < grid_blocks; ++by) {
    const MirrorOpenItem it = mirror_open_item(listed, by);
    if (it.count == 0u) {
      CHECK(it.groups == 0u && it.pad == 0u);
      CHECK(by * kMirrorQueries >= listed);
      continue;
    }
    ++working;
    CHECK(it.first == by * kMirrorQueries);
    CHECK(it.count <= kMirrorQueries && it.first + it.count <= listed);
    CHECK(it.groups >= 1u && it.groups <= kMirrorGroups);
    CHECK(32u * it.groups == it.count + it.pad && it.pad < 32u);
    for (uint32_t slot = 0; slot < 32u * it.groups; ++slot) {
      const uint32_t e = mirror_open_entry(it, slot);
      CHECK(e >= it.first && e < it.first + it.count);
      if (mirror_open_slot_live(it, slot)) {
        CHECK(e == it.first + slot);
        taken[e] += 1u;
      } else {
        CHECK(slot >= it.count && e == it.first + it.count - 1u);  // a pad slot repeats the block's last entry
      }
    }
  }
  for (uint32_t e = 0; e < listed; ++e) CHECK(taken[e] == 1u);
  CHECK(working == (listed + kMirrorQueries - 1u) / kMirrorQueries);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // ---- the open rule
  CHECK(mirror_open(1.0f, 1.0f));                           // est == thr: the row with c == thr is recorded (c <= thr)
  CHECK(mirror_open(std::nextafter(1.0f, 0.0f), 1.0f));
  CHECK(!mirror_open(std::nextafter(1.0f, 2.0f), 1.0f));
  CHECK(mirror_open(-3.0f, -3.0f) && !mirror_open(-3.0f, std::nextafter(-3.0f, -4.0f)));
  CHECK(mirror_open(5.0f, inf) && mirror_open(inf, inf));   // thr = +inf, an empty tree: open everywhere
  CHECK(mirror_open(-inf, inf));
  CHECK(!mirror_open(5.0f, -inf) && !mirror_open(inf, -inf));  // thr = -inf, a pad slot: never
  CHECK(!mirror_open(inf, 5.0f));                           // a slice past the end of the tree (est = +inf)
  CHECK(!mirror_open(nan, 1.0f) && !mirror_open(1.0f, nan) && !mirror_open(nan, inf));
  // ---- constants the kernels and the arena layout rely on
  CHECK(kMirrorQueries == 384u && kMirrorGroups * 32u == kMirrorQueries);
  // ---- counts 0, 1, 32, 33, 384, 385 (and the next block edge), on grids of one to three blocks per slice
  {
    MirrorOpenItem it = mirror_open_item(0u, 0u);
    CHECK(it.count == 0u && it.groups == 0u && it.pad == 0u);
    it = mirror_open_item(1u, 0u);
    CHECK(it.first == 0u && it.count == 1u && it.groups == 1u && it.pad == 31u);
    CHECK(mirror_open_item(1u, 1u).count == 0u);
    it = mirror_open_item(32u, 0u);
    CHECK(it.count == 32u && it.groups == 1u && it.pad == 0u);
    it = mirror_open_item(33u, 0u);
    CHECK(it.count == 33u && it.groups == 2u && it.pad == 31u);
    CHECK(mirror_open_entry(it, 32u) == 32u && mirror_open_entry(it, 33u) == 32u && mirror_open_entry(it, 63u) == 32u);
    CHECK(mirror_open_slot_live(it, 32u) && !mirror_open_slot_live(it, 33u));
    it = mirror_open_item(384u, 0u);
    CHECK(it.count == 384u && it.groups == 12u && it.pad == 0u);
    CHECK(mirror_open_item(384u, 1u).count == 0u);
    it = mirror_open_item(385u, 0u);
    CHECK(it.count == 384u && it.groups == 12u && it.pad == 0u);
    it = mirror_open_item(385u, 1u);
    CHECK(it.first == 384u && it.count == 1u && it.groups == 1u && it.pad == 31u);
    CHECK(mirror_open_entry(it, 0u) == 384u && mirror_open_entry(it, 31u) == 384u);
    CHECK(mirror_open_item(385u, 2u).count == 0u);
    it = mirror_open_item(777u, 2u);
    CHECK(it.first == 768u && it.count == 9u && it.groups == 1u && it.pad == 23u);
    it = mirror_open_item(4096u, 10u);  // the largest batch of a planner: 10 full blocks and 256
    CHECK(it.first == 3840u && it.count == 256u && it.groups == 8u && it.pad == 0u);
    CHECK(mirror_open_item(0xFFFFu, 170u).count == 255u);  // the longest list 16-bit entries can name
  }
  const uint32_t counts[] = {0u, 1u, 31u, 32u, 33u, 63u, 64u, 65u, 383u, 384u, 385u, 415u, 416u, 417u, 767u, 768u, 769u, 777u, 1152u};
  for (uint32_t listed : counts)
    for (uint32_t grid = (listed + kMirrorQueries - 1u) / kMirrorQueries; grid <= 4u; ++grid) replay(listed, grid);
  // a slice's list is never longer than the batch, so the batch's blocks per slice always cover it
  for (uint32_t B = 1; B <= 1200u; B += 7u)
    for (uint32_t open = 0; open <= B; open += (B / 5u) + 1u) {
      const uint32_t grid = (B + kMirrorQueries - 1u) / kMirrorQueries;
      CHECK(mirror_open_item(open, grid).count == 0u);
      replay(open, grid);
    }
  if (failures) {
    std::printf("nn open plan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("nn open plan ok: rule, items and pad slots\n");
  return 0;
}
