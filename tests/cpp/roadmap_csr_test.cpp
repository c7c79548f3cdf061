// Host side of the roadmap queries (reak_amd/csrc/roadmap_csr.h): the CSR builder, the predecessor walk, the path
// getter's capacity rule and the goal-side reduction.  A stand-alone program; tests/test_roadmap_queries_cpu.py compiles
// it with AddressSanitizer and UBSan and runs it.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "roadmap_csr.h"

using namespace rkh;

static int checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    ++checks;                                                       \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

// every edge is listed once under each end, in edge order, and the rows tile col exactly
static void check_csr(uint32_t n, const std::vector<uint32_t>& eu, const std::vector<uint32_t>& ev, const std::vector<double>& ew) {
  RoadmapCsr g;
  CHECK(build_roadmap_csr(n, eu.data(), ev.data(), ew.data(), ew.size(), &g));
  CHECK(g.n == n && g.row_ptr.size() == size_t(n) + 1 && g.row_ptr[0] == 0);
  CHECK(g.row_ptr[n] == 2 * ew.size() && g.col.size() == 2 * ew.size() && g.w.size() == 2 * ew.size());
  for (uint32_t v = 0; v < n; ++v) {
    CHECK(g.row_ptr[v] <= g.row_ptr[v + 1]);
    std::vector<uint32_t> want_c;
    std::vector<double> want_w;
    for (size_t e = 0; e < ew.size(); ++e) {
      if (eu[e] == v) want_c.push_back(ev[e]), want_w.push_back(ew[e]);
      if (ev[e] == v) want_c.push_back(eu[e]), want_w.push_back(ew[e]);
    }
    CHECK(g.row_ptr[v + 1] - g.row_ptr[v] == want_c.size());
    for (size_t i = 0; i < want_c.size(); ++i) {
      CHECK(g.col[g.row_ptr[v] + i] == want_c[i] && g.col[g.row_ptr[v] + i] < n);
      CHECK(g.w[g.row_ptr[v] + i] == want_w[i]);
    }
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  // ---- CSR builder
  check_csr(1, {}, {}, {});                                  // an empty edge list
  check_csr(2, {}, {}, {});                                  // two vertices with no edge
  check_csr(3, {0, 0, 1}, {1, 1, 2}, {0.5, 0.25, 1.0});      // a duplicate edge (no self-loop), different weights
  check_csr(5, {0, 1, 3}, {1, 3, 4}, {1.0, 2.0, 3.0});       // vertex 2 of degree 0 in the middle
  check_csr(6, {5, 0, 5}, {0, 4, 4}, {1.0, 0.0, 2.0});       // ids at n - 1, a zero weight
  {
    RoadmapCsr g;
    const uint32_t u[] = {0, 2}, v[] = {1, 3};
    const double w[] = {1.0, 1.0};
    CHECK(!build_roadmap_csr(3, u, v, w, 2, &g));            // an end >= n
    const uint32_t lu[] = {1}, lv[] = {1};
    CHECK(!build_roadmap_csr(3, lu, lv, w, 1, &g));          // a self-loop
  }
  // ---- predecessor walk and the capacity rule
  {
    // 0 <- 3 <- 2 <- 1 (goal); 4 unreached
    const uint32_t pred[] = {kPathNil, 2, 3, 0, kPathNil};
    const std::vector<uint32_t> p = predecessor_walk(pred, 5, 1);
    CHECK(p.size() == 4 && p[0] == 0 && p[1] == 3 && p[2] == 2 && p[3] == 1);
    CHECK(predecessor_walk(pred, 5, 4).size() == 1);         // a vertex alone
    CHECK(predecessor_walk(pred, 5, 5).empty());             // not a vertex
    const uint32_t qp[] = {kPathQueryPoint, 0, 1};           // a start connection ends the walk like the source does
    const std::vector<uint32_t> q = predecessor_walk(qp, 3, 2);
    CHECK(q.size() == 3 && q[0] == 0 && q[2] == 2);
    const uint32_t loop[] = {1, 0};                          // malformed: the walk stops after n vertices
    CHECK(predecessor_walk(loop, 2, 0).size() == 2);
    uint32_t buf[6] = {9, 9, 9, 9, 9, 9}, np = 77;
    CHECK(copy_path_out(p, nullptr, 0, &np) && np == 4);     // a length query
    np = 77;
    CHECK(!copy_path_out(p, buf, 3, &np) && np == 4 && buf[0] == 9 && buf[3] == 9);  // smaller: nothing written
    CHECK(copy_path_out(p, buf, 4, &np) && np == 4 && buf[0] == 0 && buf[3] == 1 && buf[4] == 9);   // equal
    buf[0] = buf[1] = buf[2] = buf[3] = 9;
    CHECK(copy_path_out(p, buf, 6, &np) && np == 4 && buf[1] == 3 && buf[3] == 1 && buf[4] == 9 && buf[5] == 9);  // larger
    CHECK(copy_path_out(std::vector<uint32_t>(), buf, 0, &np) && np == 0);
  }
  // ---- goal side
  {
    const double dist[] = {0.0, 0.5, 0.25, inf, 1.0};
    double cost = -1.0;
    const uint32_t v1[] = {4, 2, 1};
    const double w1[] = {0.0, 0.5, 0.25};                    // 1.0, 0.75, 0.75: the tie goes to the lower vertex
    CHECK(goal_side_min(dist, v1, w1, 3, &cost) == 1 && cost == 0.75);
    const uint32_t v2[] = {1, 2};
    CHECK(goal_side_min(dist, v2, w1 + 1, 2, &cost) == 2 && cost == 0.5);   // 1.0, 0.5
    const uint32_t v3[] = {3};
    CHECK(goal_side_min(dist, v3, w1, 1, &cost) == kPathNil && cost == inf);   // only an unreached vertex
    CHECK(goal_side_min(dist, nullptr, nullptr, 0, &cost) == kPathNil && cost == inf);   // no connection
  }
  std::printf("roadmap csr ok: %d checks\n", checks);
  return 0;
}
