// rrtstar.hip -- RRT* (unidirectional, LINEAR_SEARCH_KNN, undirected motion graph) over the quasi-static free
// space, for a batch of P independent problems:
//   rrtstar_planner::solve_planning_query_impl (ctrl/path_planning/rrtstar_path_planner.tpp:298-)
//   -> generate_rrt_star (ctrl/graph_alg/rrt_star.hpp:530-570) -> generate_rrt_star_loop (:169-190)
//   with rrg_node_generator (node_generators.hpp:137-172), star_neighborhood (neighborhood_functors.hpp:95-102),
//   lazy_node_connector (lazy_connector.hpp:79-123,230-275,332-372), pruned_node_connector::{create_pred_edge,
//   update_successors} (pruned_connector.hpp:310-332,366-382).
//
// Rewiring makes every loop iteration depend on the previous one, so iterations stay sequential; what runs on the
// device is the work *inside* an iteration, batched:
//   * the two k-NN sweeps of an iteration (knn_sweep.hip; HBM-bound at one query per tree),
//   * every candidate edge of the node generator (steer from each neighbour, the first success in order wins) and of
//     the connector (can_be_connected in both directions for every neighbour) in one edge_check launch each; the
//     sequential rules (running d_near, strict comparisons, neighbour order) are then applied on the host to the
//     precomputed verdicts, which are independent of one another.
// Every problem is a two-state machine (GENERATE: sample + k-NN + steer candidates; CONNECT: append the vertex +
// k-NN + can_be_connected candidates) and each device step serves the next state of all P problems at once
// (graph_batch.h: table-driven launches, one command upload and one result download per step).
// Bookkeeping (predecessors, accumulated distances, children lists, the DFS of update_successors) is host code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "graph_planner.h"

using namespace rkh;

namespace {
enum StarState { ST_IDLE, ST_GENERATE, ST_CONNECT, ST_CONNECT_PRED, ST_CONNECT_SUCC };

struct StarProblem {
  rkh_rrt_params prm;
  std::mt19937 eng;
  // motion graph (host)
  std::vector<double> pos;
  std::vector<uint32_t> pred;
  std::vector<double> dist, weight;
  std::vector<std::vector<uint32_t>> children;
  std::vector<uint32_t> near_seq;
  double gamma = 0.0;
  // counters
  uint64_t iteration_count = 0, samples = 0, loop_iterations = 0, num_solutions = 0, rewires = 0, edges_checked = 0;
  double best_cost = std::numeric_limits<double>::infinity();
  // state machine
  StarState state = ST_IDLE;
  std::vector<double> p_new;
  uint32_t x_near = NIL;
  double eweight = 0.0;
  int tries = 0;
  // bidirectional RRT*: the backward tree (successor links towards the goal) and the generator's second result
  std::vector<uint32_t> succ;
  std::vector<double> fwd_dist, fwd_weight;
  std::vector<std::vector<uint32_t>> parents;
  std::vector<uint32_t> near_pred, near_succ;
  std::vector<double> p_succ;
  uint32_t x_succ = NIL;
  double eweight_succ = 0.0;
  uint64_t fwd_rewires = 0, joins = 0;
  double best_join_cost = std::numeric_limits<double>::infinity();
  // branch-and-bound pruning: tombstones, the queue keyed distance_accum + distance to the goal (largest on top)
  std::vector<uint8_t> removed;
  std::vector<double> key;
  Heap4 Q;
  uint64_t pruned = 0, skipped = 0;
  double dist_to_goal = 0.0;  // of the point being connected
};
}  // namespace

struct rkh_rrtstar : GraphHandle {
  bool bidirectional = false;
  bool branch_and_bound = false;
  std::vector<StarProblem> prob;
};

namespace {

bool keep_going(const StarProblem& q) {
  return (q.iteration_count < q.prm.max_vertices) && (q.prm.max_results > q.num_solutions);
}

uint32_t add_vertex(int D, StarProblem& q, const double* pt, double d, uint32_t pr) {
  q.pos.insert(q.pos.end(), pt, pt + D);
  q.dist.push_back(d);
  q.pred.push_back(pr);
  q.weight.push_back(0.0);
  q.children.emplace_back();
  q.succ.push_back(NIL);
  q.fwd_dist.push_back(std::numeric_limits<double>::infinity());
  q.fwd_weight.push_back(0.0);
  q.parents.emplace_back();
  q.removed.push_back(0);
  q.key.push_back(0.0);
  const uint32_t v = uint32_t(q.pred.size() - 1);
  q.Q.idx(v) = size_t(-1);  // put(index_in_heap, v, -1) (branch_and_bound_connector.hpp:137,301)
  return v;
}

// vertex_to_be_removed + clear_vertex + remove_vertex: a tombstone (ids are append-only; the row on the device becomes
// +inf so that no sweep returns it, any_knn_synchro::removed_vertex).  The children of a removed vertex keep their
// predecessor field and their cost, as in the reference.
rkh_status remove_vertex(rkh_rrtstar* p, uint32_t i, uint32_t v) {
  StarProblem& q = p->prob[i];
  q.removed[v] = 1;
  ++q.pruned;
  const uint32_t pv = q.pred[v];
  if (pv != NIL && pv != v && !q.removed[pv]) {
    std::vector<uint32_t>& ch = q.children[pv];
    auto it = std::find(ch.begin(), ch.end(), v);
    if (it != ch.end()) ch.erase(it);
  }
  q.children[v].clear();
  return p->gb.remove_row(i, v);
}

void draw_sample(rkh_rrtstar* p, StarProblem& q) {
  hyperbox_point(q.eng, p->lower, p->upper, p->D, q.p_new.data());
  ++q.samples;
}

// One side of the motion graph as the connector's rules see it: the forward tree (predecessor links, cost from the
// start) or the backward tree of the bidirectional planner (successor links, cost to the goal).
struct TreeSide {
  std::vector<uint32_t>& link;               // pred / succ
  std::vector<double>& cost;                 // accumulated along the links
  std::vector<double>& weight;               // of the edge to the link
  std::vector<std::vector<uint32_t>>& adj;   // children / parents
  uint64_t& rewires;
  bool backward;  // an edge that links v into this tree runs (u -> v) in the forward tree, (v -> u) in the backward one
};
TreeSide forward_tree(StarProblem& q) { return {q.pred, q.dist, q.weight, q.children, q.rewires, false}; }
TreeSide backward_tree(StarProblem& q) { return {q.succ, q.fwd_dist, q.fwd_weight, q.parents, q.fwd_rewires, true}; }

// The newest vertex v of a problem and the verdicts of its CONNECT step: for neighbour e, verdict e is
// can_be_connected(u_e, v) and verdict K + e is can_be_connected(v, u_e); x_out is where the walk stopped, and it
// replaces the far end of the edge when the edge is weighed.
struct Connect {
  StarProblem& q;
  int D;
  uint32_t v;
  GraphBatch::Verdicts nb;
  const double* pos(uint32_t u) const { return &q.pos[size_t(u) * D]; }
  double length(bool from_v, uint32_t u) const { return from_v ? euclid(pos(v), pos(u), D) : euclid(pos(u), pos(v), D); }
  bool accepted(bool from_v, uint32_t e) const { return nb.accept[from_v ? nb.K + e : e] != 0; }
  double travelled(bool from_v, uint32_t e) const {
    return from_v ? euclid(pos(v), &nb.x_out[size_t(nb.K + e) * D], D) : euclid(pos(nb.id[e]), &nb.x_out[size_t(e) * D], D);
  }
};

// connect_best_predecessor / connect_best_successor (lazy_connector.hpp:79-123 / :125-168): the vertex of the side's
// tree through which v costs least.  *x / *ep: the generator's choice and its edge weight on entry (NIL: none)
void best_link(Connect& c, const TreeSide& s, uint32_t* x, double* ep) {
  const uint32_t orig = *x;
  double d_near = std::numeric_limits<double>::infinity();
  if (orig != NIL) d_near = s.cost[orig] + *ep;
  for (uint32_t e = 0; e < c.nb.K; ++e) {
    const uint32_t u = c.nb.id[e];
    if (u == orig || s.link[u] == NIL) continue;
    const double d = c.length(s.backward, u) + s.cost[u];
    if (d < d_near) {
      ++c.q.edges_checked;
      if (c.accepted(s.backward, e)) {
        *x = u;
        d_near = d;
        *ep = c.travelled(s.backward, e);
      }
    }
  }
}

// create_pred_edge / create_succ_edge (pruned_connector.hpp:366-382 / :388-404)
void create_link(TreeSide& s, uint32_t v, uint32_t x, double ep) {
  s.cost[v] = ep + s.cost[x];
  s.link[v] = x;
  s.weight[v] = ep;
  s.adj[x].push_back(v);
}

// connect_successors / connect_predecessors (lazy_connector.hpp:230-275 / :170-227): every neighbour that costs less
// through v is re-linked to it.  x: the link of v itself; vertices linked into the other tree are left alone; a
// removed old link (branch and bound) has no adjacency list to edit any more
void rewire_neighbours(Connect& c, TreeSide& s, const TreeSide& other, uint32_t x) {
  const uint32_t v = c.v;
  for (uint32_t e = 0; e < c.nb.K; ++e) {
    const uint32_t u = c.nb.id[e];
    if (u == x || other.link[u] != NIL) continue;
    const double d_in = c.length(!s.backward, u) + s.cost[v];
    if (d_in < s.cost[u]) {
      ++c.q.edges_checked;
      if (c.accepted(!s.backward, e)) {
        s.cost[u] = d_in;
        const uint32_t old = s.link[u];
        s.link[u] = v;
        s.weight[u] = c.travelled(!s.backward, e);
        s.adj[v].push_back(u);
        if (old != u && old != NIL && !c.q.removed[old]) {
          std::vector<uint32_t>& a = s.adj[old];
          auto it = std::find(a.begin(), a.end(), u);
          if (it != a.end()) a.erase(it);
        }
        ++s.rewires;
      }
    }
  }
}

// update_successors / update_predecessors (pruned_connector.hpp:310-332 / :338-360): the new cost of v goes down the
// adjacency lists; changed(t) for every vertex whose cost was rewritten
template <class F>
void propagate_costs(TreeSide& s, uint32_t v, F changed) {
  std::vector<uint32_t> incons(1, v);
  while (!incons.empty()) {
    const uint32_t a = incons.back();
    incons.pop_back();
    for (uint32_t t : s.adj[a]) {
      if (s.link[t] != a) continue;
      s.cost[t] = s.cost[a] + s.weight[t];
      changed(t);
      incons.push_back(t);
    }
  }
}

// lazy_node_connector::operator() (lazy_connector.hpp:332-372) on the verdicts of the CONNECT step
rkh_status connect_vertex(rkh_rrtstar* p, uint32_t i) {
  StarProblem& q = p->prob[i];
  const int D = p->D;
  Connect c{q, D, uint32_t(q.pred.size() - 1)};
  const uint32_t v = c.v;
  rkh_status st = p->gb.verdicts(i, q.pos.data(), c.pos(v), &c.nb, q.removed.data());
  if (st != RKH_OK) return st;
  TreeSide fwd = forward_tree(q), bwd = backward_tree(q);  // no vertex is ever linked into the backward tree here
  uint32_t x_near = q.x_near;
  double eweight = q.eweight;
  best_link(c, fwd, &x_near, &eweight);
  create_link(fwd, v, x_near, eweight);
  const bool bnb = p->branch_and_bound;
  if (bnb) {  // branch_and_bound_connector::operator() (branch_and_bound_connector.hpp:311-320)
    if (q.pred[1] != NIL && q.dist[v] + q.dist_to_goal > q.dist[1]) return remove_vertex(p, i, v);
    q.key[v] = q.dist[v] + q.dist_to_goal;
    q.Q.push(v);
  }
  rewire_neighbours(c, fwd, bwd, x_near);
  // with pruning (branch_and_bound_connector.hpp:142-185): the vertices whose cost changed are re-keyed (sift-up only),
  // then every vertex whose key exceeds the goal's cost is removed
  propagate_costs(fwd, v, [&](uint32_t t) {
    if (!bnb) return;
    q.key[t] = q.dist[t] + euclid(c.pos(t), c.pos(1), D);
    q.Q.push_or_update(t);
  });
  if (bnb && q.pred[1] != NIL) {
    while (!q.Q.data.empty() && q.key[q.Q.data[0]] > q.dist[1]) {
      st = remove_vertex(p, i, q.Q.data[0]);
      if (st != RKH_OK) return st;
      q.Q.pop();
    }
  }
  return RKH_OK;
}

// the bidirectional lazy_node_connector::operator() (lazy_connector.hpp:465-518) on the verdicts of a CONNECT step
rkh_status connect_vertex_bidir(rkh_rrtstar* p, uint32_t i, uint32_t x_pred, double ep_pred, uint32_t x_succ,
                                double ep_succ) {
  StarProblem& q = p->prob[i];
  Connect c{q, p->D, uint32_t(q.pred.size() - 1)};
  const uint32_t v = c.v;
  rkh_status st = p->gb.verdicts(i, q.pos.data(), c.pos(v), &c.nb);
  if (st != RKH_OK) return st;
  TreeSide fwd = forward_tree(q), bwd = backward_tree(q);
  best_link(c, fwd, &x_pred, &ep_pred);
  best_link(c, bwd, &x_succ, &ep_succ);
  if (x_pred == NIL && x_succ == NIL) return RKH_OK;  // (the reference removes the vertex here; unreachable from the loop)
  if (x_pred != NIL) create_link(fwd, v, x_pred, ep_pred);
  if (x_succ != NIL) create_link(bwd, v, x_succ, ep_succ);
  if (q.pred[v] != NIL && q.succ[v] != NIL) {  // a joining vertex (the reference registers nothing for it)
    ++q.joins;
    if (q.dist[v] + q.fwd_dist[v] < q.best_join_cost) q.best_join_cost = q.dist[v] + q.fwd_dist[v];
  }
  auto no_hook = [](uint32_t) {};
  rewire_neighbours(c, fwd, bwd, x_pred);
  propagate_costs(fwd, v, no_hook);
  rewire_neighbours(c, bwd, fwd, x_succ);
  propagate_costs(bwd, v, no_hook);
  return RKH_OK;
}

rkh_status rrtstar_create(rkh_scene* scene, const rkh_qs_space* qs, const rkh_dyn_space* dyn, const rkh_rrt_params* prms,
                          uint32_t n_problems, rkh_rrtstar** out) {
  std::vector<uint32_t> max_vertices(n_problems);
  for (uint32_t i = 0; i < n_problems; ++i) max_vertices[i] = prms[i].max_vertices;
  auto p = std::make_unique<rkh_rrtstar>();
  rkh_status st = p->init(scene, qs, dyn, max_vertices, 1, star_kmax(max_vertices));
  if (st != RKH_OK) return st;
  p->prob.resize(n_problems);
  const int D = p->D;
  for (uint32_t i = 0; i < n_problems; ++i) {
    StarProblem& q = p->prob[i];
    q.prm = prms[i];
    q.eng.seed(prms[i].seed);
    q.p_new.resize(D);
    // init_motion_graph (rrtstar_path_planner.tpp:188-203): vertex 0 = start, vertex 1 = goal;
    // generate_rrt_star (rrt_star.hpp:563-564): distance[start] = 0, predecessor[start] = start
    add_vertex(D, q, prms[i].start, 0.0, 0);
    add_vertex(D, q, prms[i].goal, std::numeric_limits<double>::infinity(), NIL);
    q.gamma = 3.0 * euclid(prms[i].start, prms[i].goal, D);  // 3 * heuristic(start -> goal) (:303,322)
  }
  st = p->append_initial_rows(2, [&](int r, uint32_t i) { return &p->prob[i].pos[size_t(r) * D]; });
  if (st != RKH_OK) return st;
  *out = p.release();
  return RKH_OK;
}

// the top of generate_rrt_star_loop (rrt_star.hpp:169-190) / generate_rrt_star_bidir_loop (:197-236): start the next
// iteration of a problem that keeps going, for at most max_loop_iterations loop passes (< 0 = unlimited)
void next_iteration(StarProblem& q, bool keep_going, int64_t max_loop_iterations) {
  if (keep_going && (max_loop_iterations < 0 || int64_t(q.loop_iterations) < max_loop_iterations)) {
    ++q.loop_iterations;
    q.tries = 0;
    q.x_near = NIL;
    q.x_succ = NIL;
    q.state = ST_GENERATE;
  } else {
    q.state = ST_IDLE;
  }
}

// The next device step of every running problem; *any = false when none is left.
//   GENERATE: sample, neighbourhood, one walk from each neighbour in order (rrg_node_generator, node_generators.hpp:
//     137-172: EDGE_STEER_ACCEPT; rrg_bidir_generator, :215-277: EDGE_STEER_BOTH).
//   CONNECT*: lazy_node_connector::operator() (lazy_connector.hpp:332-372): select_neighborhood(p) before create_vertex
//     (:347-350); then every neighbour in both directions, (u -> v) and (v -> u), for the point being connected.
rkh_status build_step(rkh_rrtstar* p, int steer_mode, bool* any) {
  GraphBatch& gb = p->gb;
  gb.begin();
  *any = false;
  for (uint32_t i = 0; i < p->P; ++i) {
    StarProblem& q = p->prob[i];
    if (q.state == ST_IDLE) continue;
    *any = true;
    uint32_t k;
    double radius;
    star_neighbourhood(q.pred.size() - size_t(q.pruned), q.gamma, p->D, &k, &radius);  // N = num_vertices(g)
    rkh_status st = RKH_OK;
    if (q.state == ST_GENERATE) {
      draw_sample(p, q);
      st = gb.cmd_knn(i, q.p_new.data(), q.pred.size(), k, radius);
      gb.cmd_edges(i, GB_LIST_KNN_TO_QUERY, 0, steer_mode, q.prm.steer_tol);
    } else {
      const double* pt = q.state == ST_CONNECT_SUCC ? q.p_succ.data() : q.p_new.data();
      const uint64_t n_before = q.pred.size();
      st = gb.cmd_knn(i, pt, n_before, k, radius);
      if (st == RKH_OK) st = gb.cmd_append(i, pt);
      gb.cmd_edges(i, GB_LIST_KNN_BIDIR, uint32_t(n_before), EDGE_CONNECT, q.prm.conn_tol);
    }
    if (st != RKH_OK) return st;
  }
  return RKH_OK;
}
}  // namespace

extern "C" {

rkh_status rkh_rrtstar_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                       uint32_t n_problems, rkh_rrtstar** out) {
  if (!scene || !space || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof || !(space->min_interval > 0.0)) {
    set_error("rkh_rrtstar_create: n_dof mismatch or min_interval <= 0");
    return RKH_ERR_BAD_ARG;
  }
  return rrtstar_create(scene, space, nullptr, prms, n_problems, out);
}

rkh_status rkh_rrtstar_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prms,
                                    uint32_t n_problems, rkh_rrtstar** out) {
  if (!scene || !space || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof) {
    set_error("rkh_rrtstar_create: n_dof mismatch");
    return RKH_ERR_BAD_ARG;
  }
  return rrtstar_create(scene, nullptr, space, prms, n_problems, out);
}

rkh_status rkh_rrtstar_destroy(rkh_rrtstar* p) {
  delete p;
  return RKH_OK;
}

// Run every problem until keep_going() is false (or max_loop_iterations loop passes, < 0 = unlimited).
rkh_status rkh_rrtstar_solve(rkh_rrtstar* p, int64_t max_loop_iterations, rkh_rrtstar_stats* stats) {
  if (!p || p->bidirectional) return RKH_ERR_BAD_ARG;
  const int D = p->D;
  const double inf = std::numeric_limits<double>::infinity();
  GraphBatch& gb = p->gb;
  auto next = [&](StarProblem& q) { next_iteration(q, keep_going(q), max_loop_iterations); };
  for (StarProblem& q : p->prob) next(q);
  for (;;) {
    bool any;
    rkh_status st = build_step(p, EDGE_STEER_ACCEPT, &any);
    if (st != RKH_OK) return st;
    if (!any) break;
    st = gb.run();
    if (st != RKH_OK) return st;
    // ---- apply the sequential rules to the verdicts
    for (uint32_t i = 0; i < p->P; ++i) {
      StarProblem& q = p->prob[i];
      if (q.state == ST_GENERATE) {
        GraphBatch::Verdicts nb;
        st = gb.verdicts(i, q.pos.data(), q.p_new.data(), &nb, q.removed.data());
        if (st != RKH_OK) return st;
        const uint32_t K = nb.K;
        const uint32_t* kidx = nb.id.data();
        const uint8_t* accept = nb.accept.data();
        const double* x_out = nb.x_out.data();
        bool was_expanded = false;
        for (uint32_t e = 0; e < K; ++e) {  // rrg_node_puller::expand_to_nearest (:61-77): first success wins
          ++q.edges_checked;
          if (accept[e]) {
            const uint32_t u = kidx[e];
            q.x_near = u;
            q.eweight = euclid(&q.pos[size_t(u) * D], &x_out[size_t(e) * D], D);  // traveled_dist
            std::memcpy(q.p_new.data(), &x_out[size_t(e) * D], D * sizeof(double));
            was_expanded = true;
            break;
          }
        }
        bool gen_done = was_expanded;
        if (!was_expanded) {
          if (q.tries >= 10) {
            gen_done = true;
            q.x_near = NIL;
          } else {
            ++q.tries;
          }
        }
        if (gen_done) {
          q.near_seq.push_back(q.x_near);
          if (q.x_near == NIL || q.dist[q.x_near] == inf) {
            next(q);  // rrt_star.hpp:181-182
          } else if (p->branch_and_bound) {
            // branch_and_bound_connector::operator() (:284-293): a point that cannot lie on a better path is dropped
            const double dist_from_start = euclid(&q.pos[0], q.p_new.data(), D);
            q.dist_to_goal = euclid(q.p_new.data(), &q.pos[size_t(1) * D], D);
            if (q.pred[1] != NIL && dist_from_start + q.dist_to_goal > q.dist[1]) {
              ++q.skipped;
              next(q);
            } else {
              q.state = ST_CONNECT;
            }
          } else {
            q.state = ST_CONNECT;
          }
        }
      } else if (q.state == ST_CONNECT) {
        add_vertex(D, q, q.p_new.data(), inf, NIL);          // rrt_conn_visitor::create_vertex
        ++q.iteration_count;                                 // vis.vertex_added -> report_progress
        if (q.pred[1] != NIL && q.dist[1] < q.best_cost) {   // dispatched_register_solution (optimal graph)
          q.best_cost = q.dist[1];
          ++q.num_solutions;
        }
        st = connect_vertex(p, i);
        if (st != RKH_OK) return st;
        next(q);
      }
    }
  }
  if (stats)
    for (uint32_t i = 0; i < p->P; ++i) {
      const StarProblem& q = p->prob[i];
      rkh_rrtstar_stats& o = stats[i];
      o.num_vertices = q.pred.size();
      o.samples = q.samples;
      o.loop_iterations = q.loop_iterations;
      o.num_solutions = q.num_solutions;
      o.rewires = q.rewires;
      o.edges_checked = q.edges_checked;
      o.best_cost = q.best_cost;
      o.pruned = q.pruned;
      o.skipped = q.skipped;
    }
  return RKH_OK;
}

// USE_BRANCH_AND_BOUND_PRUNING_FLAG (rrtstar_path_planner.tpp:270-283): generate_bnb_rrt_star instead of
// generate_rrt_star; to be chosen before the first rkh_rrtstar_solve
rkh_status rkh_rrtstar_set_branch_and_bound(rkh_rrtstar* p, int enabled) {
  if (!p || p->bidirectional) return RKH_ERR_BAD_ARG;
  for (const StarProblem& q : p->prob)
    if (q.loop_iterations != 0) {
      set_error("rkh_rrtstar_set_branch_and_bound: the planner has already run");
      return RKH_ERR_BAD_ARG;
    }
  p->branch_and_bound = enabled != 0;
  for (StarProblem& q : p->prob) {
    q.Q.greater = true;
    q.Q.key = &q.key;
  }
  return RKH_OK;
}

// removed[num_vertices]: 1 for the vertices taken out of the graph (branch-and-bound pruning)
rkh_status rkh_rrtstar_get_removed(rkh_rrtstar* p, uint32_t problem, uint8_t* removed) {
  if (!p || problem >= p->P || !removed) return RKH_ERR_BAD_ARG;
  copy_out(removed, p->prob[problem].removed);
  return RKH_OK;
}

// The current best solution: the predecessor chain of the goal vertex (vertex 1), start first
// (register_optimal_solution_path_impl, solution_path_factories.hpp:226-270).
rkh_status rkh_rrtstar_get_solution(rkh_rrtstar* p, uint32_t problem, uint32_t* path, uint32_t capacity, uint32_t* n_path,
                                    double* cost) {
  if (!p || problem >= p->P || !n_path) return RKH_ERR_BAD_ARG;
  const StarProblem& q = p->prob[problem];
  *n_path = 0;
  if (cost) *cost = q.dist[1];
  if (q.pred[1] == NIL) return RKH_OK;  // the goal is not connected
  std::vector<uint32_t> rev;
  for (uint32_t v = 1; rev.size() <= q.pred.size(); v = q.pred[v]) {
    rev.push_back(v);
    if (v == 0) break;
  }
  *n_path = uint32_t(rev.size());
  if (path) {
    if (capacity < rev.size()) {
      set_error("rkh_rrtstar_get_solution: path buffer too small");
      return RKH_ERR_CAPACITY;
    }
    for (size_t i = 0; i < rev.size(); ++i) path[i] = rev[rev.size() - 1 - i];
  }
  return RKH_OK;
}

rkh_status rkh_rrtstar_get_graph(rkh_rrtstar* p, uint32_t problem, double* pos, uint32_t* pred, double* dist,
                                 uint32_t* near_seq) {
  if (!p || problem >= p->P) return RKH_ERR_BAD_ARG;
  const StarProblem& q = p->prob[problem];
  copy_out(pos, q.pos);
  copy_out(pred, q.pred);
  copy_out(dist, q.dist);
  copy_out(near_seq, q.near_seq);
  return RKH_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Bidirectional RRT*: generate_rrt_star_bidir (rrt_star.hpp:612-659) -> generate_rrt_star_bidir_loop (:197-236) with
// rrg_bidir_generator (node_generators.hpp:215-277) and the bidirectional lazy_node_connector (lazy_connector.hpp:465-518).
// Device steps: GENERATE = sample + k-NN + one walk per neighbour (EDGE_STEER_BOTH: the verdict of
// steer_towards_position and, from the same walk, of steer_back_to_position); CONNECT = k-NN + append + both
// directions of every neighbour, once for the expanded point and once for the retracted one.
extern "C" {

rkh_status rkh_birrtstar_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                         uint32_t n_problems, rkh_rrtstar** out) {
  if (!scene || !space || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  if (space->n_dof != scene->host.n_dof || !(space->min_interval > 0.0)) {
    set_error("rkh_birrtstar_create: n_dof mismatch or min_interval <= 0");
    return RKH_ERR_BAD_ARG;
  }
  // two vertices can be added per loop iteration, the last iteration may start one short of max_vertices
  std::vector<rkh_rrt_params> grown(prms, prms + n_problems);
  for (rkh_rrt_params& g : grown) g.max_vertices += 1;
  rkh_status st = rrtstar_create(scene, space, nullptr, grown.data(), n_problems, out);
  if (st != RKH_OK) return st;
  rkh_rrtstar* p = *out;
  p->bidirectional = true;
  for (uint32_t i = 0; i < n_problems; ++i) {
    StarProblem& q = p->prob[i];
    q.prm = prms[i];
    q.p_succ.resize(p->D);
    q.fwd_dist[1] = 0.0;  // rrt_star.hpp:650-651: the goal is the root of the backward tree
    q.succ[1] = 1;
  }
  return RKH_OK;
}

rkh_status rkh_birrtstar_solve(rkh_rrtstar* p, int64_t max_loop_iterations, rkh_birrtstar_stats* stats) {
  if (!p || !p->bidirectional) return RKH_ERR_BAD_ARG;
  const int D = p->D;
  GraphBatch& gb = p->gb;
  auto next = [&](StarProblem& q) {
    next_iteration(q, q.iteration_count < q.prm.max_vertices && q.prm.max_results > 0, max_loop_iterations);
  };
  for (StarProblem& q : p->prob) next(q);
  for (;;) {
    bool any;
    rkh_status st = build_step(p, EDGE_STEER_BOTH, &any);
    if (st != RKH_OK) return st;
    if (!any) break;
    st = gb.run();
    if (st != RKH_OK) return st;
    for (uint32_t i = 0; i < p->P; ++i) {
      StarProblem& q = p->prob[i];
      if (q.state == ST_GENERATE) {
        // rrg_bidir_generator (node_generators.hpp:244-277)
        GraphBatch::Verdicts nb;
        st = gb.verdicts(i, q.pos.data(), q.p_new.data(), &nb);
        if (st != RKH_OK) return st;
        const uint32_t K = nb.K;
        const uint32_t* kidx = nb.id.data();
        const uint8_t* accept = nb.accept.data();
        const double* x_out = nb.x_out.data();
        bool was_expanded = false, was_retracted = false;
        q.x_near = NIL;
        q.x_succ = NIL;
        for (uint32_t e = 0; e < K; ++e) {  // expand_to_nearest (:84-100): neighbours of the forward tree, in order
          const uint32_t u = kidx[e];
          if (q.pred[u] == NIL) continue;
          ++q.edges_checked;
          if (accept[e] & 1) {
            q.x_near = u;
            q.eweight = euclid(&q.pos[size_t(u) * D], &x_out[size_t(e) * D], D);
            was_expanded = true;
            break;
          }
        }
        for (uint32_t e = 0; e < K; ++e) {  // retract_from_nearest (:102-118): neighbours of the backward tree
          const uint32_t u = kidx[e];
          if (q.succ[u] == NIL) continue;
          ++q.edges_checked;
          if ((accept[e] & 1) && !(accept[e] & 2)) {  // a completed walk back returns its own start: never accepted
            q.x_succ = u;
            q.eweight_succ = euclid(&x_out[size_t(e) * D], &q.pos[size_t(u) * D], D);
            std::memcpy(q.p_succ.data(), &x_out[size_t(e) * D], D * sizeof(double));
            was_retracted = true;
            break;
          }
        }
        if (was_expanded) {  // after the retraction: both pulls start from the sample
          for (uint32_t e = 0; e < K; ++e)
            if (kidx[e] == q.x_near) {
              std::memcpy(q.p_new.data(), &x_out[size_t(e) * D], D * sizeof(double));
              break;
            }
        }
        bool gen_done = was_expanded || was_retracted;
        if (!gen_done) {
          if (q.tries >= 10) gen_done = true;
          else ++q.tries;
        }
        if (gen_done) {
          q.near_pred.push_back(q.x_near);
          q.near_succ.push_back(q.x_succ);
          if (q.x_near != NIL) q.state = ST_CONNECT_PRED;
          else if (q.x_succ != NIL) q.state = ST_CONNECT_SUCC;
          else next(q);
        }
      } else if (q.state == ST_CONNECT_PRED || q.state == ST_CONNECT_SUCC) {
        const bool first = q.state == ST_CONNECT_PRED;
        add_vertex(D, q, first ? q.p_new.data() : q.p_succ.data(), std::numeric_limits<double>::infinity(), NIL);
        ++q.iteration_count;
        st = first ? connect_vertex_bidir(p, i, q.x_near, q.eweight, NIL, 0.0)
                   : connect_vertex_bidir(p, i, NIL, 0.0, q.x_succ, q.eweight_succ);
        if (st != RKH_OK) return st;
        if (first && q.x_succ != NIL) q.state = ST_CONNECT_SUCC;
        else next(q);
      }
    }
  }
  if (stats)
    for (uint32_t i = 0; i < p->P; ++i) {
      const StarProblem& q = p->prob[i];
      rkh_birrtstar_stats& o = stats[i];
      o.num_vertices = q.pred.size();
      o.samples = q.samples;
      o.loop_iterations = q.loop_iterations;
      o.rewires = q.rewires;
      o.fwd_rewires = q.fwd_rewires;
      o.joins = q.joins;
      o.edges_checked = q.edges_checked;
      o.best_join_cost = q.best_join_cost;
    }
  return RKH_OK;
}

rkh_status rkh_birrtstar_get_graph(rkh_rrtstar* p, uint32_t problem, double* pos, uint32_t* pred, double* dist, uint32_t* succ,
                                   double* fwd_dist, uint32_t* near_pred, uint32_t* near_succ) {
  if (!p || !p->bidirectional || problem >= p->P) return RKH_ERR_BAD_ARG;
  const StarProblem& q = p->prob[problem];
  copy_out(pos, q.pos);
  copy_out(pred, q.pred);
  copy_out(dist, q.dist);
  copy_out(succ, q.succ);
  copy_out(fwd_dist, q.fwd_dist);
  copy_out(near_pred, q.near_pred);
  copy_out(near_succ, q.near_succ);
  return RKH_OK;
}

}  // extern "C"
