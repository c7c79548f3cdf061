// prm.hip -- PRM (LINEAR_SEARCH_KNN, ADJ_LIST_MOTION_GRAPH, undirected motion graph) over the quasi-static free
// space, for a batch of P independent problems:
//   prm_planner::solve_planning_query (ctrl/path_planning/prm_path_planner.tpp:131-365)
//   -> generate_prm (ctrl/graph_alg/probabilistic_roadmap.hpp:309-404) -> generate_prm_impl (:211-249)
//   with prm_node_connector (prm_connector.hpp:68-182), prm_conn_visitor (probabilistic_roadmap.hpp:75-196),
//   density_plan_visitor<prm_density_calculator> (density_plan_visitors.hpp:50-224, density_calculators.hpp:45-73),
//   random_walk (planning_visitors.hpp:403-432), star_neighborhood (neighborhood_functors.hpp:95-102).
//
// The control flow of generate_prm_impl depends on the random stream (construct / expand branch, rejection
// sampling, up to 11 random-walk attempts), but the number of draws each alternative consumes is fixed, so one loop
// iteration is ONE device step (graph_batch.h) per problem:
//   construct : the next M samples are tested for is_free together; the first free one is selected on the device,
//               becomes the k-NN query and the new vertex row, and can_be_connected runs for every neighbour;
//   expand    : all 11 random-walk attempts from Q.top() are walked together; the first that travels far enough is
//               selected on the device, its end point becomes the query / new vertex, then as above.
// The host rewinds its copy of the random stream to the draw after the selected alternative, so the stream is
// consumed exactly as by the sequential reference.  Roadmap bookkeeping (4-ary indirect heap keyed by density,
// union-find of connected components, densities) is host code.
//
// Reference behaviour kept: solve_planning_query passes a density_plan_visitor (not prm_planner_visitor), whose
// publish_path tests the goal's distance_accum -- never updated on this path -- so no solution is registered and
// the roadmap grows to max_vertex_count; the start/goal component merge is reported in the stats instead.  The search
// prm_planner_visitor::publish_path (:97-122) would run is a query on the roadmap afterwards (end of this file).
// Restated third-party pieces (Boost / BGL-Extra are not in the reference tree): boost::d_ary_heap_indirect
// <V, 4, ..., std::less<double>> (push, push_or_update = insert or sift up only, pop); out_edges order of a vertex
// taken as insertion order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <set>

#include <chrono>

#include "graph_planner.h"
#include "roadmap_csr.h"
#include "roadmap_paths.h"

using namespace rkh;

namespace {
constexpr uint32_t kConstructBatch = 4;  // samples tested per construct step
constexpr uint32_t kWalkAttempts = 11;   // do { ... } while (++i <= 10)

// the global mt19937 with a replay window: speculated draws can be handed back
struct RngStream {
  std::mt19937 eng;
  std::vector<uint32_t> buf;
  size_t cur = 0;
  uint32_t operator()() {
    if (cur == buf.size()) buf.push_back(uint32_t(eng()));
    return buf[cur++];
  }
  void compact() {  // only between iterations (no stream position of a step in flight is held)
    if (cur > 65536) {
      buf.erase(buf.begin(), buf.begin() + cur);
      cur = 0;
    }
  }
};

enum PrmPending { PD_NONE, PD_CONSTRUCT, PD_EXPAND };

struct PrmProblem {
  rkh_prm_params prm;
  RngStream rng;
  // roadmap (host)
  std::vector<double> pos;
  std::vector<uint32_t> edge_u, edge_v;
  std::vector<double> edge_w;
  std::vector<std::vector<uint32_t>> incident;
  std::vector<double> density;
  std::vector<uint32_t> cc_root;
  std::set<uint32_t> cc_set;
  Heap4 Q;
  std::vector<uint8_t> kind;
  std::vector<uint32_t> expanded;
  double gamma = 0.0;
  // counters
  uint64_t iteration_count = 0, samples = 0, rejected = 0, loop_iterations = 0, publish_calls = 0, edges_checked = 0;
  int64_t merged_at_vertex = -1;
  // the step in flight
  PrmPending pending = PD_NONE;
  bool in_construct = false;  // rejection sampling of the current construct iteration continues
  uint32_t v_top = NIL;
  size_t cursor_after[kGbStageA];       // stream position if candidate c is the selected one
  size_t cursor_all_failed = 0;
  double target_dist[kGbStageA];
  bool done = false;
  uint64_t graph_version = 0;  // counts the vertices and edges added: what the roadmap queries' copies are checked against
};

// What the roadmap queries keep per problem: the CSR of the roadmap (host and device) and the search tree from vertex 0,
// each with the graph_version it was made from.
struct PrmPaths {
  RoadmapCsr csr;
  uint64_t csr_version = ~0ull, tree_version = ~0ull;
  DeviceBuffer<uint32_t> d_row, d_col;
  DeviceBuffer<double> d_w;
  std::vector<double> tree_dist;
  std::vector<uint32_t> tree_pred;
};
}  // namespace

struct rkh_prm : GraphHandle {
  std::vector<PrmProblem> prob;
  // roadmap queries (below): per-problem copies, and scratch that grows with the largest request
  std::vector<PrmPaths> paths;
  DeviceBuffer<SsspJob> d_jobs;
  DeviceBuffer<uint32_t> d_seed_v, d_pred, d_rounds, d_kidx, d_kcnt, d_nchk;
  DeviceBuffer<double> d_seed_d, d_dist, d_qpts, d_kdist, d_ea, d_eb, d_exo;
  DeviceBuffer<uint8_t> d_eacc;
  DeviceBuffer<void> d_knn_ws;
};

namespace {

bool keep_going(const PrmProblem& q) {
  return (q.iteration_count < q.prm.base.max_vertices) && (q.prm.base.max_results > 0u);
}

void random_point(rkh_prm* p, PrmProblem& q, double* out) {
  hyperbox_point(q.rng, p->lower, p->upper, p->D, out);
  ++q.samples;
}

void update_density(int D, PrmProblem& q, uint32_t u) {  // prm_density_calculator::update_density
  const size_t deg = q.incident[u].size();
  if (deg == 0) {
    q.density[u] = 0.0;
    return;
  }
  const size_t max_node_degree = size_t(D) + 1;
  double sum = 0.0;
  for (uint32_t e : q.incident[u]) sum += q.edge_w[e] / q.prm.sampling_radius;
  sum /= double(deg) * double(deg) / double(max_node_degree);
  q.density[u] = std::exp(-sum * sum);
}

void requeue(int D, PrmProblem& q, uint32_t u) {  // prm_conn_visitor::requeue_vertex
  update_density(D, q, u);
  q.Q.push_or_update(u);
}

uint32_t raw_add_vertex(int D, PrmProblem& q, const double* pt) {
  q.pos.insert(q.pos.end(), pt, pt + D);
  q.density.push_back(0.0);
  q.incident.emplace_back();
  q.cc_root.push_back(0);
  ++q.graph_version;
  return uint32_t(q.density.size() - 1);
}

void shortcut_cc_root(PrmProblem& q, uint32_t u) {  // probabilistic_roadmap.hpp:109-121
  std::vector<uint32_t> trace(1, u);
  while (q.cc_root[u] != u) {
    u = q.cc_root[u];
    trace.push_back(u);
  }
  for (uint32_t t : trace) q.cc_root[t] = u;
}

void add_edge(PrmProblem& q, uint32_t u, uint32_t v, double w) {
  const uint32_t e = uint32_t(q.edge_w.size());
  q.edge_u.push_back(u);
  q.edge_v.push_back(v);
  q.edge_w.push_back(w);
  q.incident[u].push_back(e);
  q.incident[v].push_back(e);
  ++q.graph_version;
  // prm_conn_visitor::edge_added (:123-143)
  shortcut_cc_root(q, u);
  shortcut_cc_root(q, v);
  if (q.cc_root[v] != q.cc_root[u]) {
    const uint32_t r1 = q.cc_root[u], r2 = q.cc_root[v];
    q.cc_root[r2] = r1;
    q.cc_root[v] = r1;
    q.cc_set.erase(r2);
    if (q.cc_set.size() < 2) ++q.publish_calls;
  }
  if (q.merged_at_vertex < 0) {
    uint32_t a = 0, b = 1;
    while (q.cc_root[a] != a) a = q.cc_root[a];
    while (q.cc_root[b] != b) b = q.cc_root[b];
    if (a == b) q.merged_at_vertex = int64_t(q.density.size());
  }
}

// prm_node_connector::operator() (prm_connector.hpp:136-182) on the verdicts of the finished step
rkh_status connect_vertex(rkh_prm* p, uint32_t i, const double* pt, uint32_t x_near, double eweight) {
  PrmProblem& q = p->prob[i];
  const int D = p->D;
  GraphBatch::Verdicts nb;
  rkh_status vst = p->gb.verdicts(i, q.pos.data(), pt, &nb);
  if (vst != RKH_OK) return vst;
  const uint32_t K = nb.K;
  const uint32_t* kidx = nb.id.data();
  const uint8_t* accept = nb.accept.data();
  const double* x_out = nb.x_out.data();
  // prm_conn_visitor::create_vertex (:92-107)
  const uint32_t v = raw_add_vertex(D, q, pt);
  q.cc_root[v] = v;
  q.cc_set.insert(v);
  update_density(D, q, v);
  ++q.iteration_count;
  q.Q.idx(v) = size_t(-1);
  if (x_near != NIL) {  // connect_to_first_pred (:71-91)
    add_edge(q, x_near, v, eweight);
    requeue(D, q, x_near);
  }
  requeue(D, q, v);
  for (uint32_t e = 0; e < K; ++e) {
    const uint32_t u = kidx[e];
    if (u == x_near) continue;
    ++q.edges_checked;
    if (accept[e]) add_edge(q, u, v, euclid(&q.pos[size_t(u) * D], &x_out[size_t(e) * D], D));
    requeue(D, q, u);
  }
  requeue(D, q, v);
  return RKH_OK;
}

rkh_status prm_create(rkh_scene* scene, const rkh_qs_space* space, const rkh_dyn_space* dyn, const rkh_prm_params* prms,
                      uint32_t n_problems, rkh_prm** out) {
  std::vector<uint32_t> max_vertices(n_problems);
  for (uint32_t i = 0; i < n_problems; ++i) {
    if (!(prms[i].sampling_radius > 0.0)) {
      set_error("rkh_prm_create: sampling_radius must be positive");
      return RKH_ERR_BAD_ARG;
    }
    max_vertices[i] = prms[i].base.max_vertices;
  }
  auto p = std::make_unique<rkh_prm>();
  rkh_status st = p->init(scene, space, dyn, max_vertices, 1, star_kmax(max_vertices));
  if (st != RKH_OK) return st;
  const int D = p->D;
  p->prob.resize(n_problems);
  p->paths.resize(n_problems);
  for (uint32_t i = 0; i < n_problems; ++i) {
    PrmProblem& q = p->prob[i];
    q.prm = prms[i];
    q.rng.eng.seed(prms[i].base.seed);
    q.Q.key = &q.density;
    // RK_PRM_PLANNER_INITIALIZE_START_AND_GOAL, then generate_prm on a non-empty graph (:368-397)
    raw_add_vertex(D, q, prms[i].base.start);
    raw_add_vertex(D, q, prms[i].base.goal);
    for (uint32_t u = 0; u < 2; ++u) {
      update_density(D, q, u);
      q.Q.push(u);
      q.cc_root[u] = u;
    }
    q.cc_set.insert(0);
    q.cc_set.insert(1);
    q.gamma = 3.0 * euclid(prms[i].base.start, prms[i].base.goal, D);
  }
  st = p->append_initial_rows(2, [&](int r, uint32_t i) { return &p->prob[i].pos[size_t(r) * D]; });
  if (st != RKH_OK) return st;
  *out = p.release();
  return RKH_OK;
}
}  // namespace

extern "C" {

rkh_status rkh_prm_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_prm_params* prms,
                                   uint32_t n_problems, rkh_prm** out) {
  if (!scene || !space || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof || !(space->min_interval > 0.0)) {
    set_error("rkh_prm_create: n_dof mismatch or min_interval <= 0");
    return RKH_ERR_BAD_ARG;
  }
  return prm_create(scene, space, nullptr, prms, n_problems, out);
}

rkh_status rkh_prm_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_prm_params* prms, uint32_t n_problems,
                                rkh_prm** out) {
  if (!scene || !space || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof) {
    set_error("rkh_prm_create: n_dof mismatch");
    return RKH_ERR_BAD_ARG;
  }
  return prm_create(scene, nullptr, space, prms, n_problems, out);
}

rkh_status rkh_prm_destroy(rkh_prm* p) {
  delete p;
  return RKH_OK;
}

// Run every problem until keep_going() is false (or max_loop_iterations loop passes, < 0 = unlimited).
rkh_status rkh_prm_solve(rkh_prm* p, int64_t max_loop_iterations, rkh_prm_stats* stats) {
  if (!p) return RKH_ERR_BAD_ARG;
  const int D = p->D;
  GraphBatch& gb = p->gb;
  for (;;) {
    gb.begin();
    bool any = false;
    for (uint32_t i = 0; i < p->P; ++i) {
      PrmProblem& q = p->prob[i];
      q.pending = PD_NONE;
      if (!q.in_construct) {
        // top of the while (vis.keep_going()) loop of generate_prm_impl
        if (!(keep_going(q) && (max_loop_iterations < 0 || int64_t(q.loop_iterations) < max_loop_iterations))) continue;
        ++q.loop_iterations;
        q.rng.compact();
        const double rand_value = uniform_01(q.rng);
        if (rand_value > q.prm.expand_probability) {
          q.in_construct = true;
        } else if (q.Q.data.empty()) {
          set_error("rkh_prm_solve: expansion queue ran empty (the reference calls top() on an empty heap here)");
          return RKH_ERR_CAPACITY;
        } else {
          q.pending = PD_EXPAND;
        }
      }
      any = true;
      GbAux& a = gb.h_aux[i];
      const size_t N = q.density.size();
      uint32_t k;
      double radius;
      star_neighbourhood(N, q.gamma, D, &k, &radius);
      rkh_status st;
      if (q.in_construct) {
        // construction node (:229-235): the next kConstructBatch samples of the rejection loop
        q.pending = PD_CONSTRUCT;
        for (uint32_t c = 0; c < kConstructBatch; ++c) {
          random_point(p, q, a.pts[c]);
          q.cursor_after[c] = q.rng.cur;
        }
        st = gb.cmd_stage_a(i, GB_SELECT_POINT, kConstructBatch, 0, 0.0);
      } else {
        // expansion node (:237-246): the 11 attempts of random_walk (planning_visitors.hpp:403-432) from Q.top()
        const uint32_t v = q.Q.data[0];
        q.v_top = v;
        q.expanded.push_back(v);
        const double* pv = &q.pos[size_t(v) * D];
        double p_rnd[RKH_MAX_DOF], dp[RKH_MAX_DOF];
        random_point(p, q, p_rnd);
        for (int d = 0; d < D; ++d) dp[d] = p_rnd[d] - (p->lower[d] + 0.5 * (p->upper[d] - p->lower[d]));
        for (uint32_t c = 0; c < kWalkAttempts; ++c) {
          for (int d = 0; d < D; ++d) a.pts[c][d] = pv[d] + dp[d];
          const double dist = euclid(pv, a.pts[c], D);
          const double target_dist = uniform_01(q.rng) * q.prm.sampling_radius;
          a.frac[c] = target_dist / dist;
          a.target_dist[c] = target_dist;
          q.target_dist[c] = target_dist;
          q.cursor_after[c] = q.rng.cur;
          random_point(p, q, p_rnd);  // drawn by the failure branch of this attempt
          for (int d = 0; d < D; ++d) dp[d] = p_rnd[d] - (p->lower[d] + 0.5 * (p->upper[d] - p->lower[d]));
        }
        q.cursor_all_failed = q.rng.cur;
        st = gb.cmd_stage_a(i, GB_SELECT_WALK, kWalkAttempts, v, q.prm.base.steer_tol);
      }
      if (st == RKH_OK) st = gb.cmd_knn(i, a.pts[0], N, k, radius);  // the query is written by the select kernel
      if (st != RKH_OK) return st;
      gb.cmd_edges(i, GB_LIST_KNN_TO_VERTEX, uint32_t(N), EDGE_CONNECT, q.prm.base.conn_tol);
    }
    if (!any) break;
    rkh_status st = gb.run();
    if (st != RKH_OK) return st;
    for (uint32_t i = 0; i < p->P; ++i) {
      PrmProblem& q = p->prob[i];
      if (q.pending == PD_NONE) continue;
      const uint32_t sel = gb.selected(i);
      if (q.pending == PD_CONSTRUCT) {
        if (sel == NIL) {  // all rejected: the rejection loop goes on with the next samples
          q.rejected += kConstructBatch;
          continue;
        }
        // hand the samples after the accepted one back to the stream
        q.samples -= (kConstructBatch - 1 - sel);
        q.rejected += sel;
        q.rng.cur = q.cursor_after[sel];
        gb.confirm_selected(i);
        double pt[RKH_MAX_DOF];
        std::memcpy(pt, gb.h_aux[i].pts[sel], D * sizeof(double));
        st = connect_vertex(p, i, pt, NIL, 0.0);
        if (st != RKH_OK) return st;
        q.kind.push_back(0);
        q.expanded.push_back(NIL);
        q.in_construct = false;
      } else {
        if (sel == NIL) {  // random_walk failed: Q.pop()
          q.edges_checked += kWalkAttempts;
          q.rng.cur = q.cursor_all_failed;
          q.Q.pop();
          q.kind.push_back(2);
          continue;
        }
        q.edges_checked += sel + 1;
        q.samples -= (kWalkAttempts - sel);  // samples of the attempts that were never made
        q.rng.cur = q.cursor_after[sel];
        gb.confirm_selected(i);
        double pt[RKH_MAX_DOF];
        std::memcpy(pt, gb.a_x_out(i) + size_t(sel) * D, D * sizeof(double));
        const double traveled = euclid(&q.pos[size_t(q.v_top) * D], pt, D);
        st = connect_vertex(p, i, pt, q.v_top, traveled);
        if (st != RKH_OK) return st;
        q.kind.push_back(1);
      }
    }
  }
  if (stats)
    for (uint32_t i = 0; i < p->P; ++i) {
      const PrmProblem& q = p->prob[i];
      rkh_prm_stats& o = stats[i];
      o.num_vertices = q.density.size();
      o.num_edges = q.edge_w.size();
      o.samples = q.samples;
      o.rejected = q.rejected;
      o.loop_iterations = q.loop_iterations;
      o.num_components = q.cc_set.size();
      o.publish_calls = q.publish_calls;
      o.merged_at_vertex = q.merged_at_vertex;
      o.edges_checked = q.edges_checked;
      o.device_steps = p->gb.steps;
    }
  return RKH_OK;
}

rkh_status rkh_prm_get_graph(rkh_prm* p, uint32_t problem, double* pos, uint32_t* edge_u, uint32_t* edge_v,
                             double* edge_w, double* density, uint32_t* cc_root, uint8_t* kind, uint32_t* expanded) {
  if (!p || problem >= p->P) return RKH_ERR_BAD_ARG;
  const PrmProblem& q = p->prob[problem];
  copy_out(pos, q.pos);
  copy_out(edge_u, q.edge_u);
  copy_out(edge_v, q.edge_v);
  copy_out(edge_w, q.edge_w);
  copy_out(density, q.density);
  copy_out(cc_root, q.cc_root);
  copy_out(kind, q.kind);
  copy_out(expanded, q.expanded);
  return RKH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Roadmap queries (rkh.h): the search prm_planner_visitor::publish_path runs (prm_path_planner.tpp:97-122), as a query
// on the roadmap as it stands.  The searches are roadmap_paths.hip's, on the handle's stream; the CSR of a problem is
// rebuilt and uploaded only when its roadmap has changed since the copy was made.
namespace {

template <class T>
rkh_status grow(DeviceBuffer<T>& b, size_t n) {
  return n > b.size() ? b.alloc(n) : RKH_OK;
}

rkh_status ensure_csr(rkh_prm* p, uint32_t i) {
  const PrmProblem& q = p->prob[i];
  PrmPaths& c = p->paths[i];
  if (c.csr_version == q.graph_version) return RKH_OK;
  c.csr_version = ~0ull;
  if (!build_roadmap_csr(uint32_t(q.density.size()), q.edge_u.data(), q.edge_v.data(), q.edge_w.data(), q.edge_w.size(), &c.csr)) {
    set_error("roadmap query: the roadmap's edge list is not a simple graph over its vertices");
    return RKH_ERR_UNSUPPORTED;
  }
  hipStream_t s = p->gb.stream;
  const size_t nnz = c.csr.col.size();
  RKH_TRY(grow(c.d_row, c.csr.row_ptr.size()));
  RKH_TRY(grow(c.d_col, std::max<size_t>(nnz, 1)));
  RKH_TRY(grow(c.d_w, std::max<size_t>(nnz, 1)));
  RKH_HIP(hipMemcpyAsync(c.d_row.get(), c.csr.row_ptr.data(), c.csr.row_ptr.size() * 4, hipMemcpyHostToDevice, s));
  if (nnz) {
    RKH_HIP(hipMemcpyAsync(c.d_col.get(), c.csr.col.data(), nnz * 4, hipMemcpyHostToDevice, s));
    RKH_HIP(hipMemcpyAsync(c.d_w.get(), c.csr.w.data(), nnz * 8, hipMemcpyHostToDevice, s));
  }
  RKH_HIP(hipStreamSynchronize(s));
  c.csr_version = q.graph_version;
  return RKH_OK;
}

// The searches from roadmap vertices, pairs[j] = (problem, source vertex): job table, seeds and output rows on the
// device (row j of d_dist / d_pred starts at off[j]; d_rounds[j]), ready for launch_roadmap_sssp(.., n_max).
struct VertexSearches {
  std::vector<size_t> off;
  uint32_t n_max = 0;
};
rkh_status prepare_vertex_searches(rkh_prm* p, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, VertexSearches* out) {
  const size_t J = pairs.size();
  out->off.assign(J + 1, 0);
  out->n_max = 0;
  for (size_t j = 0; j < J; ++j) {
    RKH_TRY(ensure_csr(p, pairs[j].first));
    const uint32_t n = p->paths[pairs[j].first].csr.n;
    out->off[j + 1] = out->off[j] + n;
    out->n_max = std::max(out->n_max, n);
  }
  hipStream_t s = p->gb.stream;
  RKH_TRY(grow(p->d_seed_v, J));
  RKH_TRY(grow(p->d_seed_d, J));
  RKH_TRY(grow(p->d_dist, out->off[J]));
  RKH_TRY(grow(p->d_pred, out->off[J]));
  RKH_TRY(grow(p->d_rounds, J));
  RKH_TRY(grow(p->d_jobs, J));
  std::vector<uint32_t> seed_v(J);
  std::vector<SsspJob> jobs(J);
  for (size_t j = 0; j < J; ++j) {
    const PrmPaths& c = p->paths[pairs[j].first];
    seed_v[j] = pairs[j].second;
    SsspJob& job = jobs[j];
    job.row_ptr = c.d_row.get();
    job.col = c.d_col.get();
    job.w = c.d_w.get();
    job.n = c.csr.n;
    job.n_seeds = 1;
    job.seed_v = p->d_seed_v.get() + j;
    job.seed_d = p->d_seed_d.get() + j;
    job.seed_mark = NIL;
    job.dist = p->d_dist.get() + out->off[j];
    job.pred = p->d_pred.get() + out->off[j];
    job.rounds = p->d_rounds.get() + j;
  }
  RKH_HIP(hipMemcpyAsync(p->d_seed_v.get(), seed_v.data(), J * 4, hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemsetAsync(p->d_seed_d.get(), 0, J * 8, s));  // every seed distance is 0.0
  RKH_HIP(hipMemcpyAsync(p->d_jobs.get(), jobs.data(), J * sizeof(SsspJob), hipMemcpyHostToDevice, s));
  RKH_HIP(hipStreamSynchronize(s));  // the host copies end here
  return RKH_OK;
}

// the tree from vertex 0 of every problem whose roadmap changed since its tree was made: one launch, one workgroup each
rkh_status refresh_trees(rkh_prm* p) {
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  for (uint32_t i = 0; i < p->P; ++i)
    if (p->paths[i].tree_version != p->prob[i].graph_version) pairs.push_back(std::make_pair(i, 0u));
  if (pairs.empty()) return RKH_OK;
  VertexSearches vs;
  RKH_TRY(prepare_vertex_searches(p, pairs, &vs));
  hipStream_t s = p->gb.stream;
  RKH_TRY(launch_roadmap_sssp(s, p->d_jobs.get(), uint32_t(pairs.size()), vs.n_max));
  for (size_t j = 0; j < pairs.size(); ++j) {
    PrmPaths& c = p->paths[pairs[j].first];
    c.tree_version = ~0ull;
    c.tree_dist.resize(c.csr.n);
    c.tree_pred.resize(c.csr.n);
    RKH_HIP(hipMemcpyAsync(c.tree_dist.data(), p->d_dist.get() + vs.off[j], size_t(c.csr.n) * 8, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipMemcpyAsync(c.tree_pred.data(), p->d_pred.get() + vs.off[j], size_t(c.csr.n) * 4, hipMemcpyDeviceToHost, s));
  }
  RKH_HIP(hipStreamSynchronize(s));
  for (size_t j = 0; j < pairs.size(); ++j) p->paths[pairs[j].first].tree_version = p->prob[pairs[j].first].graph_version;
  return RKH_OK;
}

}  // namespace

extern "C" {

rkh_status rkh_prm_shortest_paths(rkh_prm* p, uint32_t problem, const uint32_t* sources, uint32_t S, double* dist,
                                  uint32_t* pred) {
  if (!p || problem >= p->P || (!dist && !pred)) return RKH_ERR_BAD_ARG;
  if (S == 0) return RKH_OK;
  if (!sources) return RKH_ERR_BAD_ARG;
  const size_t n = p->prob[problem].density.size();
  std::vector<std::pair<uint32_t, uint32_t>> pairs(S);
  for (uint32_t j = 0; j < S; ++j) {
    if (sources[j] >= n) {
      set_error("rkh_prm_shortest_paths: a source is not a vertex of the roadmap");
      return RKH_ERR_BAD_ARG;
    }
    pairs[j] = std::make_pair(problem, sources[j]);
  }
  VertexSearches vs;
  RKH_TRY(prepare_vertex_searches(p, pairs, &vs));
  hipStream_t s = p->gb.stream;
  RKH_TRY(launch_roadmap_sssp(s, p->d_jobs.get(), S, vs.n_max));
  if (dist) RKH_HIP(hipMemcpyAsync(dist, p->d_dist.get(), size_t(S) * n * 8, hipMemcpyDeviceToHost, s));
  if (pred) RKH_HIP(hipMemcpyAsync(pred, p->d_pred.get(), size_t(S) * n * 4, hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  return RKH_OK;
}

// start (vertex 0) -> goal (vertex 1): the predecessor walk from the goal, as register_optimal_solution_path_impl
// (solution_path_factories.hpp:226-270) would walk it; capacity / NULL / n_path rules of rkh_rrtstar_get_solution
rkh_status rkh_prm_get_solution(rkh_prm* p, uint32_t problem, uint32_t* path, uint32_t capacity, uint32_t* n_path,
                                double* cost) {
  if (!p || problem >= p->P || !n_path) return RKH_ERR_BAD_ARG;
  RKH_TRY(refresh_trees(p));
  const PrmPaths& c = p->paths[problem];
  *n_path = 0;
  if (cost) *cost = c.tree_dist[1];
  if (std::isinf(c.tree_dist[1])) return RKH_OK;  // the goal is not connected
  if (!copy_path_out(predecessor_walk(c.tree_pred.data(), c.csr.n, 1), path, capacity, n_path)) {
    set_error("rkh_prm_get_solution: path buffer too small");
    return RKH_ERR_CAPACITY;
  }
  return RKH_OK;
}

rkh_status rkh_prm_query_paths(rkh_prm* p, uint32_t problem, const double* starts, const double* goals, uint32_t B, uint32_t k,
                               double radius, uint32_t capacity, double* cost, uint32_t* path, uint32_t* n_path) {
  if (!p || problem >= p->P) return RKH_ERR_BAD_ARG;
  if (p->gb.dynamic) {
    set_error("rkh_prm_query_paths: quasi-static roadmaps only (the connections of a dynamic roadmap are directional propagations)");
    return RKH_ERR_UNSUPPORTED;
  }
  if (B == 0) return RKH_OK;
  if (!starts || !goals || !cost || !n_path || k == 0 || B > 0x7FFFFFFFu / k / 2u) return RKH_ERR_BAD_ARG;
  const PrmProblem& q = p->prob[problem];
  GraphBatch& gb = p->gb;
  const int D = p->D;
  const uint32_t n = uint32_t(q.density.size()), Q = 2 * B;
  if (gb.prob[problem].n_dev != n) {
    set_error("rkh_prm_query_paths: the device rows do not match the roadmap");
    return RKH_ERR_DEVICE;
  }
  RKH_TRY(ensure_csr(p, problem));
  hipStream_t s = gb.stream;
  // 1. neighbourhoods: one k-NN launch for the 2B points (starts, then goals) over the problem's device rows
  KnnWorkspace ws;
  size_t ws_bytes = 0;
  RKH_TRY(knn_plan_or_error(n, Q, k, &ws, &ws_bytes, knn_list_cap_from_env()));
  RKH_TRY(grow(p->d_knn_ws, ws_bytes));
  knn_carve(p->d_knn_ws.get(), Q, &ws);
  RKH_TRY(grow(p->d_qpts, size_t(Q) * D));
  RKH_TRY(grow(p->d_kidx, size_t(Q) * k));
  RKH_TRY(grow(p->d_kdist, size_t(Q) * k));
  RKH_TRY(grow(p->d_kcnt, Q));
  RKH_HIP(hipMemcpyAsync(p->d_qpts.get(), starts, size_t(B) * D * 8, hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemcpyAsync(p->d_qpts.get() + size_t(B) * D, goals, size_t(B) * D * 8, hipMemcpyHostToDevice, s));
  RKH_TRY(launch_nnk(s, gb.prob[problem].tree, n, p->d_qpts.get(), Q, k, radius, p->d_kidx.get(), p->d_kdist.get(),
                     p->d_kcnt.get(), ws));
  std::vector<uint32_t> kidx(size_t(Q) * k), kcnt(Q);
  std::vector<double> kdist(size_t(Q) * k);
  // a first pass whose bound named more vertices than a list holds is followed by the exact retry (knn_plan.h)
  for (int pass = 0;; ++pass) {
    uint32_t overflow = 0;  // first word of the k-NN workspace
    RKH_HIP(hipMemcpyAsync(kidx.data(), p->d_kidx.get(), kidx.size() * 4, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipMemcpyAsync(kdist.data(), p->d_kdist.get(), kdist.size() * 8, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipMemcpyAsync(kcnt.data(), p->d_kcnt.get(), size_t(Q) * 4, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipMemcpyAsync(&overflow, p->d_knn_ws.get(), 4, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipStreamSynchronize(s));
    if (!overflow) break;
    if (pass == 1) {
      set_error(std::string("rkh_prm_query_paths: ") + knn_capacity_text());
      return RKH_ERR_CAPACITY;
    }
    RKH_TRY(launch_nnk_retry(s, gb.prob[problem].tree, n, p->d_qpts.get(), Q, k, radius, p->d_kidx.get(),
                             p->d_kdist.get(), p->d_kcnt.get(), ws));
  }
  // 2. connections: every candidate edge in the direction of travel (start -> u, u -> goal), one edge-walk launch.  A point
  //    that coincides with a roadmap vertex is connected to it with weight 0 (a walk of no length is never accepted).
  struct Conn {
    uint32_t point, v;  // point: index into the 2B points
    double w;
    int64_t edge;       // its walk, or -1: accepted as it is
  };
  std::vector<Conn> conns;
  std::vector<double> ea, eb;
  for (uint32_t pt = 0; pt < Q; ++pt) {
    const double* x = (pt < B ? starts + size_t(pt) * D : goals + size_t(pt - B) * D);
    for (uint32_t e = 0; e < std::min(kcnt[pt], k); ++e) {
      const uint32_t v = kidx[size_t(pt) * k + e];
      if (v >= n) continue;
      Conn c = {pt, v, 0.0, -1};
      if (kdist[size_t(pt) * k + e] != 0.0) {
        c.edge = int64_t(ea.size() / D);
        const double* xv = &q.pos[size_t(v) * D];
        ea.insert(ea.end(), pt < B ? x : xv, (pt < B ? x : xv) + D);
        eb.insert(eb.end(), pt < B ? xv : x, (pt < B ? xv : x) + D);
      }
      conns.push_back(c);
    }
  }
  const uint32_t E = uint32_t(ea.size() / D);
  std::vector<uint8_t> eacc(E);
  std::vector<double> exo(size_t(E) * D);
  if (E) {
    RKH_TRY(grow(p->d_ea, ea.size()));
    RKH_TRY(grow(p->d_eb, eb.size()));
    RKH_TRY(grow(p->d_exo, ea.size()));
    RKH_TRY(grow(p->d_nchk, E));
    RKH_TRY(grow(p->d_eacc, E));
    RKH_HIP(hipMemcpyAsync(p->d_ea.get(), ea.data(), ea.size() * 8, hipMemcpyHostToDevice, s));
    RKH_HIP(hipMemcpyAsync(p->d_eb.get(), eb.data(), eb.size() * 8, hipMemcpyHostToDevice, s));
    EdgeIO io;
    io.src = p->d_ea.get();
    io.src_stride = D;
    io.tgt = p->d_eb.get();
    io.tgt_stride = D;
    io.B = E;
    io.x_out = p->d_exo.get();
    io.steps_free = p->d_nchk.get();
    io.accept = p->d_eacc.get();
    io.mode = EDGE_CONNECT;  // can_be_connected, with the problem's connection tolerance
    io.steer_tol = q.prm.base.conn_tol;
    io.err_flag = gb.scene->d_err.get();
    RKH_TRY(launch_edge_check(s, *gb.scene, gb.qs, io, E));
    RKH_HIP(hipMemcpyAsync(eacc.data(), p->d_eacc.get(), E, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipMemcpyAsync(exo.data(), p->d_exo.get(), exo.size() * 8, hipMemcpyDeviceToHost, s));
    RKH_HIP(hipStreamSynchronize(s));
  }
  // the accepted ones, weighted as connect_vertex weights a roadmap edge: |first point of the walk - its end point|
  std::vector<std::vector<uint32_t>> conn_v(Q);
  std::vector<std::vector<double>> conn_w(Q);
  for (const Conn& c : conns) {
    double w = 0.0;
    if (c.edge >= 0) {
      if (!eacc[c.edge]) continue;
      w = euclid(&ea[size_t(c.edge) * D], &exo[size_t(c.edge) * D], D);
    }
    conn_v[c.point].push_back(c.v);
    conn_w[c.point].push_back(w);
  }
  // 3. searches: the accepted start connections of pair b are the seed list of search b; one launch
  std::vector<uint32_t> seed_v;
  std::vector<double> seed_d;
  std::vector<size_t> seed_off(B + 1, 0);
  for (uint32_t b = 0; b < B; ++b) {
    seed_v.insert(seed_v.end(), conn_v[b].begin(), conn_v[b].end());
    seed_d.insert(seed_d.end(), conn_w[b].begin(), conn_w[b].end());
    seed_off[b + 1] = seed_v.size();
  }
  const PrmPaths& c = p->paths[problem];
  RKH_TRY(grow(p->d_seed_v, std::max<size_t>(seed_v.size(), 1)));
  RKH_TRY(grow(p->d_seed_d, std::max<size_t>(seed_d.size(), 1)));
  RKH_TRY(grow(p->d_dist, size_t(B) * n));
  RKH_TRY(grow(p->d_pred, size_t(B) * n));
  RKH_TRY(grow(p->d_jobs, B));
  std::vector<SsspJob> jobs(B);
  for (uint32_t b = 0; b < B; ++b) {
    SsspJob& job = jobs[b];
    job.row_ptr = c.d_row.get();
    job.col = c.d_col.get();
    job.w = c.d_w.get();
    job.n = n;
    job.n_seeds = uint32_t(seed_off[b + 1] - seed_off[b]);
    job.seed_v = p->d_seed_v.get() + seed_off[b];
    job.seed_d = p->d_seed_d.get() + seed_off[b];
    job.seed_mark = RKH_PRM_QUERY_POINT;
    job.dist = p->d_dist.get() + size_t(b) * n;
    job.pred = p->d_pred.get() + size_t(b) * n;
  }
  if (!seed_v.empty()) {
    RKH_HIP(hipMemcpyAsync(p->d_seed_v.get(), seed_v.data(), seed_v.size() * 4, hipMemcpyHostToDevice, s));
    RKH_HIP(hipMemcpyAsync(p->d_seed_d.get(), seed_d.data(), seed_d.size() * 8, hipMemcpyHostToDevice, s));
  }
  RKH_HIP(hipMemcpyAsync(p->d_jobs.get(), jobs.data(), size_t(B) * sizeof(SsspJob), hipMemcpyHostToDevice, s));
  RKH_TRY(launch_roadmap_sssp(s, p->d_jobs.get(), B, n));
  std::vector<double> dist(size_t(B) * n);
  std::vector<uint32_t> pred(size_t(B) * n);
  RKH_HIP(hipMemcpyAsync(dist.data(), p->d_dist.get(), dist.size() * 8, hipMemcpyDeviceToHost, s));
  RKH_HIP(hipMemcpyAsync(pred.data(), p->d_pred.get(), pred.size() * 4, hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  // 4. goal side, on the host
  for (uint32_t b = 0; b < B; ++b) {
    const std::vector<uint32_t>& gv = conn_v[B + b];
    const uint32_t last = goal_side_min(&dist[size_t(b) * n], gv.data(), conn_w[B + b].data(), gv.size(), &cost[b]);
    n_path[b] = 0;
    if (last == kPathNil) continue;
    const std::vector<uint32_t> walk = predecessor_walk(&pred[size_t(b) * n], n, last);
    n_path[b] = uint32_t(walk.size());
    if (path)
      for (size_t i = 0; i < walk.size() && i < capacity; ++i) path[size_t(b) * capacity + i] = walk[i];
  }
  return RKH_OK;
}

// rkh_diag.h: the search launch alone between events, and the host Dijkstra it is compared with
rkh_status rkh_diag_prm_search_ms(rkh_prm* p, uint32_t problem, const uint32_t* sources, uint32_t S, uint32_t runs, float* ms,
                                  uint32_t* max_rounds, double* host_ms) {
  if (!p || !ms || runs == 0 || (problem != 0xFFFFFFFFu && (problem >= p->P || !sources || S == 0))) return RKH_ERR_BAD_ARG;
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  if (problem == 0xFFFFFFFFu) {
    for (uint32_t i = 0; i < p->P; ++i) pairs.push_back(std::make_pair(i, 0u));
  } else {
    for (uint32_t j = 0; j < S; ++j) {
      if (sources[j] >= p->prob[problem].density.size()) return RKH_ERR_BAD_ARG;
      pairs.push_back(std::make_pair(problem, sources[j]));
    }
  }
  VertexSearches vs;
  RKH_TRY(prepare_vertex_searches(p, pairs, &vs));
  hipStream_t s = p->gb.stream;
  const uint32_t J = uint32_t(pairs.size());
  hipEvent_t e0 = nullptr, e1 = nullptr;
  RKH_HIP(hipEventCreate(&e0));
  RKH_HIP(hipEventCreate(&e1));
  rkh_status st = launch_roadmap_sssp(s, p->d_jobs.get(), J, vs.n_max);  // warm-up
  for (uint32_t r = 0; st == RKH_OK && r < runs; ++r) {
    hipError_t e = hipEventRecord(e0, s);
    if (e == hipSuccess) st = launch_roadmap_sssp(s, p->d_jobs.get(), J, vs.n_max);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms[r], e0, e1);
    if (e != hipSuccess && st == RKH_OK) {
      set_error(std::string("rkh_diag_prm_search_ms: ") + hipGetErrorString(e));
      st = RKH_ERR_DEVICE;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  RKH_TRY(st);
  std::vector<uint32_t> rounds(J);
  RKH_HIP(hipMemcpy(rounds.data(), p->d_rounds.get(), size_t(J) * 4, hipMemcpyDeviceToHost));
  if (max_rounds) *max_rounds = *std::max_element(rounds.begin(), rounds.end());
  if (host_ms) {
    std::vector<double> d;
    const auto t0 = std::chrono::steady_clock::now();
    for (const auto& pr : pairs) host_dijkstra(p->paths[pr.first].csr, pr.second, &d);
    *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return RKH_OK;
}

}  // extern "C"
