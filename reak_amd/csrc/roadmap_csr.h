// roadmap_csr.h -- host side of the roadmap queries (prm.hip, roadmap_paths.hip): the CSR adjacency of an undirected
// roadmap, the predecessor walk that turns a search tree into a path, and the goal-side rule of a multi-query.  No HIP
// and no device type in here, so a host compiler and a sanitizer can read it alone (tests/cpp/roadmap_csr_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace rkh {

constexpr uint32_t kPathNil = 0xFFFFFFFFu;         // no predecessor: the source vertex, or a vertex the search did not reach
constexpr uint32_t kPathQueryPoint = 0xFFFFFFFEu;  // RKH_PRM_QUERY_POINT: the predecessor is the query point itself

// Adjacency of an undirected graph of n vertices: the neighbours of v are col[row_ptr[v] .. row_ptr[v + 1]) with weights
// w[..], in the order of the edge list; every edge (u, v, w) appears once under u and once under v (a duplicate edge
// twice under each).  Edges must join distinct vertices below n.
struct RoadmapCsr {
  uint32_t n = 0;
  std::vector<uint32_t> row_ptr, col;
  std::vector<double> w;
};

// false: an edge with an end >= n, a self-loop, or more than 2^31 - 1 edges (row_ptr holds 32-bit offsets)
inline bool build_roadmap_csr(uint32_t n, const uint32_t* edge_u, const uint32_t* edge_v, const double* edge_w, size_t n_edges,
                              RoadmapCsr* out) {
  if (n_edges > size_t(0x7FFFFFFF)) return false;
  out->n = n;
  out->row_ptr.assign(size_t(n) + 1, 0u);
  out->col.assign(2 * n_edges, 0u);
  out->w.assign(2 * n_edges, 0.0);
  for (size_t e = 0; e < n_edges; ++e) {
    if (edge_u[e] >= n || edge_v[e] >= n || edge_u[e] == edge_v[e]) return false;
    ++out->row_ptr[size_t(edge_u[e]) + 1];
    ++out->row_ptr[size_t(edge_v[e]) + 1];
  }
  for (uint32_t v = 0; v < n; ++v) out->row_ptr[size_t(v) + 1] += out->row_ptr[v];
  std::vector<uint32_t> fill(out->row_ptr.begin(), out->row_ptr.end() - 1);
  for (size_t e = 0; e < n_edges; ++e) {
    const uint32_t u = edge_u[e], v = edge_v[e];
    out->col[fill[u]] = v;
    out->w[fill[u]++] = edge_w[e];
    out->col[fill[v]] = u;
    out->w[fill[v]++] = edge_w[e];
  }
  return true;
}

// The predecessor walk from `last` (solution_path_factories.hpp walks the goal's predecessors the same way): the vertices
// from the one whose predecessor is no roadmap vertex (kPathNil: the source; kPathQueryPoint: a start connection) to
// `last`, in travel order.  At most n vertices are taken, so a malformed pred array cannot loop.  Empty: last >= n.
inline std::vector<uint32_t> predecessor_walk(const uint32_t* pred, uint32_t n, uint32_t last) {
  std::vector<uint32_t> rev;
  for (uint32_t v = last; v < n && rev.size() < n; v = pred[v]) rev.push_back(v);
  return std::vector<uint32_t>(rev.rbegin(), rev.rend());
}

// What a path getter hands out (the rule of rkh_rrtstar_get_solution): *n_path = the length; with a buffer, all of the
// path or -- capacity too small -- nothing and false.
inline bool copy_path_out(const std::vector<uint32_t>& path, uint32_t* out, uint32_t capacity, uint32_t* n_path) {
  *n_path = uint32_t(path.size());
  if (!out) return true;
  if (capacity < path.size()) return false;
  for (size_t i = 0; i < path.size(); ++i) out[i] = path[i];
  return true;
}

// Goal side of a multi-query: cost = min over the accepted goal connections (conn_v[i], conn_w[i]) of
// dist[conn_v[i]] + conn_w[i]; the lowest vertex wins ties.  Returns that vertex, or kPathNil (cost +inf) when no
// connection ends at a reached vertex.
inline uint32_t goal_side_min(const double* dist, const uint32_t* conn_v, const double* conn_w, size_t n_conn, double* cost) {
  uint32_t best = kPathNil;
  double c = std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < n_conn; ++i) {
    const double t = dist[conn_v[i]] + conn_w[i];
    if (std::isinf(t)) continue;
    if (t < c || (t == c && conn_v[i] < best)) {
      c = t;
      best = conn_v[i];
    }
  }
  *cost = c;
  return best;
}

}  // namespace rkh
