// knn_plan.h -- the launch plan and the workspace of the k-NN search (knn_sweep.hip), stated once for the kernels, their
// callers (rkh_api_nn.hip, prm.hip, graph_batch.hip) and a host compiler: nothing here uses HIP, so
// tests/cpp/knn_plan_test.cpp reads this header as it is and runs the plan under a sanitizer without a GPU.
//
// The search (knn_sweep.hip): a bound sweep leaves m_sub = gx * ksel row-subset minima per query, tau is the k-th
// smallest of them, a collect sweep appends every vertex with d <= tau and d < radius to the query's list of cmax
// slots, a select kernel sorts the list and writes the first k.
//
// THE GUARANTEE.  The first pass is a bound, not a promise: tau is +inf when fewer than k subset minima are finite
// (m_sub < k: few tiles and a large k; or live rows in fewer than k blocks after removals), and a loose tau can name
// more than cmax vertices.  A query whose list overflowed (cnt > cmax) is then served by the EXACT RETRY: one block
// finds the k-th smallest distance inside the radius by bisection over the bits of a double, counting only, and the
// normal collect and select run again for that query alone with tau = that distance.  The retry needs no workspace
// beyond `bytes` and is launched only after an overflow was seen.  Its list holds the k nearest and every further
// vertex at exactly the k-th distance: a request with 1 <= k <= 1024 fails (RKH_ERR_CAPACITY) only if more than
// knn_tie_room(ws, k) vertices besides the k nearest lie at exactly the k-th distance (coincident vertices).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rkh.h"

namespace rkh {

constexpr int kKnnTileRows = 256;
constexpr int kKnnThreads = 256;
constexpr int kKnnSelMax = 8;        // a block contributes the ksel <= 8 smallest of its row-subset minima per query
constexpr uint32_t kKnnMaxK = 1024;
constexpr uint32_t kKnnSortMax = 4096;  // entries the LDS sorts of knn_tau_kernel / knn_select_kernel take
constexpr size_t kKnnBatchWsBytes = 128 * 1024;  // what a graph batch keeps per problem (one query: B = 1)

struct KnnWorkspace {
  double* sub = nullptr;       // [M][Bpad] per-subrange minima (phase A)
  double* tau = nullptr;       // [B] inclusive bound on the k-th smallest distance
  uint32_t* cnt = nullptr;     // [B] candidates collected
  double* cand_d = nullptr;    // [B][cmax]
  uint32_t* cand_i = nullptr;  // [B][cmax]
  uint32_t* overflow = nullptr;
  uint32_t cmax = 0, m_sub = 0, gx = 0;
  uint32_t ksel = 8;           // subset minima a block contributes per query (1..8)
};

inline int knn_query_block(uint32_t B) { return B <= 8 ? 8 : 32; }  // queries per block

inline uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

inline uint64_t knn_tiles(uint64_t n) { return (n + kKnnTileRows - 1) / kKnnTileRows; }
// tiles a block of the sweep owns (blocks past the last tile own none)
inline uint64_t knn_tiles_per_block(uint64_t n, uint32_t gx) { return (knn_tiles(n) + gx - 1) / gx; }

// RKH_ERR_BAD_ARG: k outside [1, 1024] (nothing is written).
inline rkh_status knn_plan(uint64_t n, uint32_t B, uint32_t k, KnnWorkspace* ws, size_t* bytes) {
  if (k == 0 || k > kKnnMaxK) return RKH_ERR_BAD_ARG;
  const uint32_t qb = uint32_t(knn_query_block(B));
  const uint32_t gy = (B + qb - 1) / qb;
  uint64_t tiles = knn_tiles(n);
  if (tiles < 1) tiles = 1;
  // enough subsets for a tight bound (M >= 4k) and enough blocks to fill the chip, but M <= 4096 (LDS sort)
  uint64_t gx = (4ull * k + kKnnSelMax - 1) / kKnnSelMax;  // >= 1
  const uint64_t fill = 2048 / (gy ? gy : 1u);
  if (gx < fill) gx = fill;
  if (gx > tiles) gx = tiles;
  if (gx > kKnnSortMax / kKnnSelMax) gx = kKnnSortMax / kKnnSelMax;
  ws->gx = uint32_t(gx);
  // about 4k subset minima in total are plenty for a tight bound (the k-th smallest of M minima leaves ~ -M ln(1 - k/M)
  // candidates); fewer minima = a shorter sort in knn_tau_kernel
  uint32_t ksel = uint32_t((4ull * k + gx - 1) / gx);
  if (ksel < 1) ksel = 1;
  if (ksel > uint32_t(kKnnSelMax)) ksel = kKnnSelMax;
  ws->ksel = ksel;
  ws->m_sub = uint32_t(gx) * ksel;
  ws->cmax = next_pow2(8 * k);
  if (ws->cmax < 2048) ws->cmax = 2048;
  if (ws->cmax > kKnnSortMax) ws->cmax = kKnnSortMax;
  *bytes = 256 + size_t(ws->m_sub) * B * 8 + size_t(B) * 8 + size_t(B) * 4 + size_t(B) * ws->cmax * 12 + 64;
  return RKH_OK;
}

inline void knn_carve(void* base, uint32_t B, KnnWorkspace* ws) {
  unsigned char* p = static_cast<unsigned char*>(base);
  ws->overflow = reinterpret_cast<uint32_t*>(p);
  p += 256;
  ws->sub = reinterpret_cast<double*>(p);
  p += size_t(ws->m_sub) * B * 8;
  ws->tau = reinterpret_cast<double*>(p);
  p += size_t(B) * 8;
  ws->cand_d = reinterpret_cast<double*>(p);
  p += size_t(B) * ws->cmax * 8;
  ws->cand_i = reinterpret_cast<uint32_t*>(p);
  p += size_t(B) * ws->cmax * 4;
  ws->cnt = reinterpret_cast<uint32_t*>(p);
}

// ---- the guarantee, as predicates of the plan
// The bound sweep cannot bound the k-th distance at all (tau = +inf whatever the data): the collect sweep then takes
// every vertex inside the radius.
inline bool knn_first_pass_unbounded(const KnnWorkspace& ws, uint32_t k) { return ws.m_sub < k; }
// ... and with more than cmax rows that can overflow the list: the requests the first pass alone had to refuse.
inline bool knn_needs_exact_retry(uint64_t n, uint32_t k, const KnnWorkspace& ws) {
  return knn_first_pass_unbounded(ws, k) && n > ws.cmax;
}
// Vertices at exactly the k-th distance, besides the k nearest, that the exact retry's list still holds.
inline uint32_t knn_tie_room(const KnnWorkspace& ws, uint32_t k) { return ws.cmax - k; }

}  // namespace rkh
