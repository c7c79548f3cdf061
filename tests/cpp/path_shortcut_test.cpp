// path_shortcut_test.cpp -- the index rules of reak_amd/csrc/path_shortcut.h, compiled by the host compiler with
// AddressSanitizer and UBSan and run directly (tests/test_path_shortcut_cpu.py): the pair index is a bijection onto
// [0, count) in the order i ascending, then j ascending, for L = 1 .. 70 and the spans 0, 1, 2, L - 1, L, L + 3; the count
// agrees with the enumeration; the allowed rule; the predecessor walk, also over garbage.
#include <cstdio>
#include <vector>

#include "path_shortcut.h"

using namespace rkh;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int main() {
  unsigned long long pairs_seen = 0;
  for (uint32_t L = 1; L <= 70; ++L) {
    const uint32_t spans[6] = {0, 1, 2, L - 1, L, L + 3};
    for (uint32_t max_span : spans) {
      const uint32_t span = (max_span == 0 || max_span > L - 1) ? L - 1 : max_span;
      CHECK(shortcut_span(L, max_span) == span);
      // the enumeration of the definition: i ascending, then j ascending, 1 <= j - i <= span
      std::vector<std::pair<uint32_t, uint32_t> > want;
      for (uint32_t i = 0; i < L; ++i)
        for (uint32_t j = i + 1; j < L && j - i <= span; ++j) want.push_back(std::make_pair(i, j));
      CHECK(shortcut_pair_count(L, max_span) == want.size());
      std::vector<uint32_t> hit(want.size(), 0);  // sized exactly: an index out of range is an ASan report
      for (size_t p = 0; p < want.size(); ++p) {
        const uint32_t idx = shortcut_pair_index(L, max_span, want[p].first, want[p].second);
        CHECK(idx == p);
        if (idx < hit.size()) ++hit[idx];
        uint32_t i = 0xFFFFFFFFu, j = 0xFFFFFFFFu;
        shortcut_pair_at(L, max_span, uint32_t(p), &i, &j);
        CHECK(i == want[p].first && j == want[p].second);
        ++pairs_seen;
      }
      for (uint32_t h : hit) CHECK(h == 1);
    }
  }
  // the largest path: the count fits 32 bits and the last pair is the last index
  CHECK(shortcut_pair_count(kShortcutMaxPoints, 0) == 523776ull);
  CHECK(shortcut_pair_index(kShortcutMaxPoints, 0, kShortcutMaxPoints - 2, kShortcutMaxPoints - 1) == 523775u);
  CHECK(shortcut_pair_count(kShortcutMaxPoints, 3) == 3ull * 1021 + 3);
  CHECK(shortcut_pair_count(0, 0) == 0 && shortcut_pair_count(1, 5) == 0);
  {
    uint32_t i = 0, j = 0;
    shortcut_pair_at(kShortcutMaxPoints, 0, 523775u, &i, &j);
    CHECK(i == kShortcutMaxPoints - 2 && j == kShortcutMaxPoints - 1);
  }
  // allowed: consecutive hops always; longer hops need the verdict and the span
  CHECK(shortcut_allowed(3, 4, 1, false) && shortcut_allowed(3, 4, 5, true));
  CHECK(!shortcut_allowed(3, 5, 5, false) && shortcut_allowed(3, 5, 2, true) && !shortcut_allowed(3, 6, 2, true));
  // the predecessor walk
  {
    const uint32_t pred[6] = {kShortcutNil, 0, 0, 1, 2, 2};
    std::vector<uint32_t> rev(6, 77);
    CHECK(shortcut_walk(pred, 6, rev.data()) == 3 && rev[0] == 5 && rev[1] == 2 && rev[2] == 0 && rev[3] == 77);
    CHECK(shortcut_walk(pred, 1, rev.data()) == 1 && rev[0] == 0);
    CHECK(shortcut_walk(pred, 0, rev.data()) == 0);
    const uint32_t chain[5] = {kShortcutNil, 0, 1, 2, 3};
    std::vector<uint32_t> full(5);
    CHECK(shortcut_walk(chain, 5, full.data()) == 5 && full[4] == 0 && full[0] == 4);
    // garbage ends the walk inside the buffer: a predecessor that is not below its vertex
    const uint32_t bad[4] = {kShortcutNil, 1, 3, 2};
    std::vector<uint32_t> r4(4);
    CHECK(shortcut_walk(bad, 4, r4.data()) == 2 && r4[0] == 3 && r4[1] == 2);
  }
  if (failures) return 1;
  std::printf("path shortcut ok: %llu pairs\n", pairs_seen);
  return 0;
}
