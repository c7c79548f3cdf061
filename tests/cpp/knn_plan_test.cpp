// The launch plan and the workspace of the k-NN search (reak_amd/csrc/knn_plan.h) over a grid of requests, on the host:
// built with AddressSanitizer and UBSan by tests/test_knn_plan_cpu.py and run directly.  The header uses no HIP.
//
// `knn_plan_test` checks the grid and prints "knn plan ok: ...".  `knn_plan_test N B K` prints the plan of one request
// (the GPU tests and DESIGN.md 4.4 take from it which requests the first pass alone cannot serve).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_plan.h"

using namespace rkh;

static int failures = 0;
#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      std::printf("FAILED %s:%d: %s  (n=%llu B=%u k=%u)\n", __FILE__, __LINE__, #cond,                  \
                  (unsigned long long)g_n, g_B, g_k);                                                   \
      ++failures;                                                                                       \
    }                                                                                                   \
  } while (0)

static uint64_t g_n = 0;
static uint32_t g_B = 0, g_k = 0;

static bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }

static void check_request(uint64_t n, uint32_t B, uint32_t k) {
  g_n = n, g_B = B, g_k = k;
  KnnWorkspace ws;
  size_t bytes = 0;
  CHECK(knn_plan(n, B, k, &ws, &bytes) == RKH_OK);
  const uint64_t tiles = knn_tiles(n);
  const uint32_t qb = uint32_t(knn_query_block(B));
  CHECK(qb == (B <= 8 ? 8u : 32u));
  // the grid: every tile has a block, no more blocks than tiles
  CHECK(ws.gx >= 1 && ws.gx <= std::max<uint64_t>(tiles, 1));
  CHECK(ws.gx <= 512);
  CHECK(uint64_t(ws.gx) * knn_tiles_per_block(n, ws.gx) >= tiles);
  // a block has 256 / QB row subsets per query and hands on at most 8 of their minima
  CHECK(ws.ksel >= 1 && ws.ksel <= std::min<uint32_t>(8, 256 / qb));
  CHECK(ws.m_sub == ws.gx * ws.ksel);
  CHECK(ws.m_sub <= 4096);                   // the LDS sort of knn_tau_kernel
  CHECK(next_pow2(ws.m_sub) <= kKnnSortMax);
  CHECK(is_pow2(ws.cmax) && ws.cmax <= 4096 && ws.cmax >= 2048);  // the LDS sort of knn_select_kernel
  // the guarantee (knn_plan.h): a list that the first pass overflowed is redone by the exact retry, whose list must hold
  // the k nearest and has room for further vertices at exactly the k-th distance; where the first pass cannot bound the
  // k-th distance at all and the rows outnumber a list, the request is served by that retry (and was refused before)
  CHECK(ws.cmax >= 4 * k);
  CHECK(knn_tie_room(ws, k) >= 3 * k && knn_tie_room(ws, k) >= 1024);
  CHECK(knn_needs_exact_retry(n, k, ws) == (ws.m_sub < k && n > ws.cmax));
  CHECK(ws.m_sub >= k || n <= ws.cmax || knn_needs_exact_retry(n, k, ws));
  if (knn_needs_exact_retry(n, k, ws)) CHECK(8 * tiles < k || ws.gx * 8u < k);
  // the carve: disjoint extents in [0, bytes), doubles 8-byte aligned
  std::vector<unsigned char> arena(bytes + 16);
  unsigned char* base = arena.data() + ((16 - (reinterpret_cast<uintptr_t>(arena.data()) & 15u)) & 15u);
  knn_carve(base, B, &ws);
  struct Extent {
    const unsigned char* p;
    size_t len;
    bool doubles;
  };
  const Extent ext[] = {
      {reinterpret_cast<const unsigned char*>(ws.overflow), 4, false},
      {reinterpret_cast<const unsigned char*>(ws.sub), size_t(ws.m_sub) * B * 8, true},
      {reinterpret_cast<const unsigned char*>(ws.tau), size_t(B) * 8, true},
      {reinterpret_cast<const unsigned char*>(ws.cand_d), size_t(B) * ws.cmax * 8, true},
      {reinterpret_cast<const unsigned char*>(ws.cand_i), size_t(B) * ws.cmax * 4, false},
      {reinterpret_cast<const unsigned char*>(ws.cnt), size_t(B) * 4, false},
  };
  const size_t n_ext = sizeof(ext) / sizeof(ext[0]);
  for (size_t i = 0; i < n_ext; ++i) {
    CHECK(ext[i].p >= base && ext[i].p + ext[i].len <= base + bytes);
    CHECK((reinterpret_cast<uintptr_t>(ext[i].p) - reinterpret_cast<uintptr_t>(base)) % (ext[i].doubles ? 8 : 4) == 0);
    for (size_t j = i + 1; j < n_ext; ++j)
      CHECK(ext[i].p + ext[i].len <= ext[j].p || ext[j].p + ext[j].len <= ext[i].p);
  }
  if (B == 1) CHECK(bytes <= kKnnBatchWsBytes);  // what a graph batch keeps per problem
}

int main(int argc, char** argv) {
  if (argc == 4) {
    const uint64_t n = std::strtoull(argv[1], nullptr, 10);
    const uint32_t B = uint32_t(std::strtoul(argv[2], nullptr, 10)), k = uint32_t(std::strtoul(argv[3], nullptr, 10));
    KnnWorkspace ws;
    size_t bytes = 0;
    if (knn_plan(n, B, k, &ws, &bytes) != RKH_OK) return 2;
    std::printf("n=%llu B=%u k=%u tiles=%llu gx=%u ksel=%u m_sub=%u cmax=%u bytes=%zu unbounded=%d needs_retry=%d\n",
                (unsigned long long)n, B, k, (unsigned long long)knn_tiles(n), ws.gx, ws.ksel, ws.m_sub, ws.cmax, bytes,
                int(knn_first_pass_unbounded(ws, k)), int(knn_needs_exact_retry(n, k, ws)));
    return 0;
  }
  const uint64_t ns[] = {0, 1, 255, 256, 257, 2048, 2049, 2304, 3000, 8192, 32767, 32768, 131072, 153600, 1ull << 20};
  const uint32_t Bs[] = {1, 8, 9, 32, 33, 257};
  const uint32_t ks[] = {1, 2, 8, 72, 73, 100, 256, 257, 1024};
  unsigned checked = 0, retry = 0;
  for (uint64_t n : ns)
    for (uint32_t B : Bs)
      for (uint32_t k : ks) {
        check_request(n, B, k);
        KnnWorkspace ws;
        size_t bytes = 0;
        (void)knn_plan(n, B, k, &ws, &bytes);
        retry += knn_needs_exact_retry(n, k, ws) ? 1u : 0u;
        ++checked;
      }
  // the two requests the plan was read for: 12 tiles x 8 minima < 100
  {
    g_n = 3000, g_B = 1, g_k = 100;
    KnnWorkspace ws;
    size_t bytes = 0;
    CHECK(knn_plan(3000, 1, 100, &ws, &bytes) == RKH_OK);
    CHECK(ws.gx == 12 && ws.ksel == 8 && ws.m_sub == 96 && ws.cmax == 2048 && knn_needs_exact_retry(3000, 100, ws));
    CHECK(knn_plan(40000, 20, 24, &ws, &bytes) == RKH_OK);
    CHECK(ws.gx == 157 && ws.ksel == 1 && !knn_needs_exact_retry(40000, 24, ws));  // bounded, unless rows are removed
    CHECK(knn_plan(153600, 7, 16, &ws, &bytes) == RKH_OK);
    CHECK(ws.gx == 512 && knn_tiles(153600) == 600 && knn_tiles_per_block(153600, ws.gx) == 2);  // blocks 300.. own no tile
  }
  // k outside [1, 1024] is refused and writes nothing
  {
    g_n = 1000, g_B = 1;
    KnnWorkspace ws;
    size_t bytes = 12345;
    g_k = 0;
    CHECK(knn_plan(1000, 1, 0, &ws, &bytes) == RKH_ERR_BAD_ARG);
    g_k = 1025;
    CHECK(knn_plan(1000, 1, 1025, &ws, &bytes) == RKH_ERR_BAD_ARG);
    CHECK(bytes == 12345 && ws.gx == 0 && ws.cmax == 0);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("knn plan ok: %u requests, %u served by the exact retry alone\n", checked, retry);
  return 0;
}
