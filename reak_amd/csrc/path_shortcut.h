// path_shortcut.h -- the index rules of path shortcutting (path_shortcut.hip; the definitions are at rkh_shortcut_paths in
// include/rkh.h), each once: which vertex pairs of a path are candidates, where pair (i, j) sits in the pair arrays and
// back, which pairs the search may use, and the predecessor walk that turns the search's result into the kept vertices.
// No HIP header and no device builtin: a host compiler and a sanitizer read it on a machine without a GPU
// (tests/cpp/path_shortcut_test.cpp).
//
// A path of L >= 1 points has the candidates (i, j), 0 <= i < j <= L - 1, j - i <= span, in the order i ascending, then j
// ascending.  With s = shortcut_span(L, max_span) the rows i <= L - 1 - s hold s pairs each and start at i * s; behind them
// the rows shrink by one pair each, down to the single pair (L - 2, L - 1).
#pragma once
#include <cstdint>

#ifndef RKH_HD
#ifdef __HIPCC__
#define RKH_HD __host__ __device__ __forceinline__
#else
#define RKH_HD inline
#endif
#endif

namespace rkh {

constexpr uint32_t kShortcutMaxPoints = 1024;         // points of one path (the search keeps a path's vertices in one workgroup)
constexpr uint64_t kShortcutMaxPairs = 0x7FFFFFFFull; // candidate pairs of one call (one edge walk each, one launch)
constexpr uint32_t kShortcutNil = 0xFFFFFFFFu;

// the span in effect: max_span == 0 means every pair; no pair is longer than the path
RKH_HD uint32_t shortcut_span(uint32_t L, uint32_t max_span) {
  const uint32_t whole = L ? L - 1 : 0;
  return (max_span == 0 || max_span > whole) ? whole : max_span;
}

// candidate pairs of a path: (L - s) full rows of s, then s - 1, s - 2, ..., 1
RKH_HD uint64_t shortcut_pair_count(uint32_t L, uint32_t max_span) {
  const uint64_t s = shortcut_span(L, max_span);
  return s ? (uint64_t(L) - s) * s + s * (s - 1) / 2 : 0;
}

// pairs in the t shrinking rows behind row L - s (row L - s + u holds s - 1 - u pairs)
RKH_HD uint32_t shortcut_tail_start(uint32_t s, uint32_t t) { return t * (s - 1) - t * (t - 1) / 2; }

// where pair (i, j) sits; requires i < j < L and j - i <= shortcut_span(L, max_span), L <= kShortcutMaxPoints
RKH_HD uint32_t shortcut_pair_index(uint32_t L, uint32_t max_span, uint32_t i, uint32_t j) {
  const uint32_t s = shortcut_span(L, max_span);
  if (i <= L - s) return i * s + (j - i - 1);
  return (L - s) * s + shortcut_tail_start(s, i - (L - s)) + (j - i - 1);
}

// and back: the pair at index p < shortcut_pair_count(L, max_span)
RKH_HD void shortcut_pair_at(uint32_t L, uint32_t max_span, uint32_t p, uint32_t* i, uint32_t* j) {
  const uint32_t s = shortcut_span(L, max_span);
  const uint32_t full = (L - s) * s;
  if (p < full) {
    *i = p / s;
    *j = *i + 1 + p % s;
    return;
  }
  const uint32_t q = p - full;
  uint32_t lo = 0, hi = s - 1;  // the row t with tail_start(t) <= q < tail_start(t + 1); rows 0 .. s - 2 hold a pair
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (shortcut_tail_start(s, mid) <= q) lo = mid;
    else hi = mid;
  }
  *i = L - s + lo;
  *j = *i + 1 + (q - shortcut_tail_start(s, lo));
}

// May the search hop from i to j > i?  Consecutive hops are the caller's path: always.  A longer hop needs the strict
// verdict of its walk, and lies within the span.
RKH_HD bool shortcut_allowed(uint32_t i, uint32_t j, uint32_t span, bool ok) {
  return j == i + 1 || (ok && j - i <= span);
}

// The predecessor walk from vertex L - 1: rev[0] = L - 1, rev[1] = pred[L - 1], ... down to vertex 0; returns the number
// of vertices written (the kept path is rev read backwards).  pred[v] < v for every v the search reached; a pred that is
// not (kShortcutNil, or an index not below v) ends the walk, so it takes at most L steps whatever pred holds.
RKH_HD uint32_t shortcut_walk(const uint32_t* pred, uint32_t L, uint32_t* rev) {
  if (L == 0) return 0;
  uint32_t n = 0, v = L - 1;
  for (;;) {
    rev[n++] = v;
    if (v == 0 || pred[v] >= v) break;
    v = pred[v];
  }
  return n;
}

}  // namespace rkh
