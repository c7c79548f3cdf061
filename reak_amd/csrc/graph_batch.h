// graph_batch.h -- device plumbing shared by the motion-graph planners whose loop iterations are sequential
// (RRT*, PRM): P independent problems, each a small state machine on the host; one "step" of every problem
// (append a vertex row -> k-NN of one point -> candidate edge list from the k-NN result -> quasi-static edge
// walk of every candidate) runs as ONE set of launches for all problems (device tables, blockIdx.z / .y =
// problem) with one command upload and one result download -- the cost of a step does not grow with P until
// the chip is full.  The sequential rules of the reference (neighbour order, strict comparisons, running
// minima) are applied by the host to the downloaded, mutually independent verdicts.  The kernels and the method
// bodies are in graph_batch.hip.
//
// Reference pieces served: star_neighborhood + min_dist_linear_search k-NN (ctrl/graph_alg/neighborhood_functors.hpp:95-102,
// ctrl/path_planning/topological_search.hpp:244-274); steer_towards_position / can_be_connected over the
// quasi-static free space (ctrl/path_planning/planning_visitors.hpp:349-360,385-395 ->
// ctrl/interpolation/interpolated_topologies.hpp:137-163 -> manip_free_workspace.hpp:154-156).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "rkh_internal.h"

namespace rkh {

enum GbListMode : uint32_t {
  GB_LIST_NONE = 0,          // no edges this step
  GB_LIST_KNN_TO_QUERY = 1,  // (u -> query point) for every k-NN result u, in k-NN order
  GB_LIST_KNN_BIDIR = 2,     // (u -> v) for every u, then (v -> u) for every u
  GB_LIST_KNN_TO_VERTEX = 3, // (u -> v) for every u
};

constexpr uint32_t kGbStageA = 16;  // candidate points / walks of the first stage

enum GbSelect : uint32_t {
  GB_SELECT_NONE = 0,
  GB_SELECT_POINT = 1,  // the first accepted stage-A candidate point becomes the query point and the new vertex row
  GB_SELECT_WALK = 2,   // the end point of the first accepted stage-A walk becomes the query point and the new vertex row
};

struct GbAux {  // per-problem command fields read by the prep / select / list kernels
  double query[RKH_MAX_DOF];
  double append_row[RKH_MAX_DOF];
  double* append_dst;      // null: nothing to append
  // stage A (PRM): candidate points / random-walk targets, tested before the k-NN of the same step
  double pts[kGbStageA][RKH_MAX_DOF];
  double frac[kGbStageA];
  double target_dist[kGbStageA];
  uint32_t a_src[kGbStageA];
  uint32_t a_count;
  uint32_t select_mode;    // GbSelect
  double* select_dst;      // row the selected point is appended to
  const uint8_t* a_accept; // stage-A verdicts / end points (device result block)
  const double* a_xout;
  uint32_t* sel;           // selected candidate or 0xFFFFFFFF (device result block)
  uint32_t list_mode;
  uint32_t v;              // vertex id used by the list modes
  const uint32_t* kidx;    // k-NN result (device)
  const uint32_t* kcnt;
  uint32_t* src_idx;       // edge lists (device)
  uint32_t* tgt_idx;
  uint32_t* n_edges;       // device-side edge count (read by the edge kernel)
};

// boost::d_ary_heap_indirect<Vertex, 4, IndexInHeapMap, KeyMap, Compare> restated from its published definition (push,
// push_or_update = insert-or-sift-UP-only, pop, top).  greater = false: std::less (PRM's density queue, smallest key on
// top); greater = true: std::greater (branch_and_bound_connector's queue, largest key on top).
struct Heap4 {
  bool greater = false;
  bool before(double a, double b) const { return greater ? a > b : a < b; }
  std::vector<uint32_t> data;
  std::vector<size_t> index;
  const std::vector<double>* key = nullptr;
  size_t& idx(uint32_t v) {
    if (index.size() <= v) index.resize(size_t(v) + 1, 0);
    return index[v];
  }
  void sift_up(size_t i) {
    if (i == 0) return;
    const size_t orig = i;
    const uint32_t moving = data[i];
    const double moving_key = (*key)[moving];
    size_t levels = 0;
    while (i != 0) {
      const size_t parent = (i - 1) / 4;
      if (before(moving_key, (*key)[data[parent]])) {
        ++levels;
        i = parent;
      } else {
        break;
      }
    }
    i = orig;
    for (size_t l = 0; l < levels; ++l) {
      const size_t parent = (i - 1) / 4;
      const uint32_t pv = data[parent];
      idx(pv) = i;
      data[i] = pv;
      i = parent;
    }
    data[i] = moving;
    idx(moving) = i;
  }
  void sift_down() {
    if (data.empty()) return;
    size_t i = 0;
    const double moving_key = (*key)[data[0]];
    const size_t n = data.size();
    for (;;) {
      const size_t first = 4 * i + 1;
      if (first >= n) break;
      const size_t nc = (first + 4 <= n) ? 4 : n - first;
      size_t best = 0;
      double best_key = (*key)[data[first]];
      for (size_t c = 1; c < nc; ++c) {
        const double k = (*key)[data[first + c]];
        if (before(k, best_key)) {
          best = c;
          best_key = k;
        }
      }
      if (before(best_key, moving_key)) {
        const size_t c = first + best;
        std::swap(data[c], data[i]);
        idx(data[i]) = i;
        idx(data[c]) = c;
        i = c;
      } else {
        break;
      }
    }
  }
  void push(uint32_t v) {
    const size_t i = data.size();
    data.push_back(v);
    idx(v) = i;
    sift_up(i);
  }
  void push_or_update(uint32_t v) {
    size_t i = idx(v);
    if (i == size_t(-1)) {
      i = data.size();
      data.push_back(v);
      idx(v) = i;
    }
    sift_up(i);
  }
  void pop() {
    idx(data[0]) = size_t(-1);
    if (data.size() != 1) {
      data[0] = data.back();
      idx(data[0]) = 0;
      data.pop_back();
      sift_down();
    } else {
      data.pop_back();
    }
  }
};

struct GbProblem {
  DeviceBuffer<double> pos;      // the vertex rows
  NnStore tree;                  // ... as the launchers take them
  uint64_t n_dev = 0;            // rows on the device
  DeviceBuffer<void> d_knn_ws;
  DeviceBuffer<uint32_t> d_src_idx, d_tgt_idx;
};

struct GraphBatch {
  rkh_scene* scene = nullptr;
  hipStream_t stream = nullptr;
  QsDev qs;
  bool dynamic = false;  // edges are RK4 propagations through the steerable dynamic space (D = 2 n_dof states)
  DynDev dyn;
  SteerRequest steer_req;  // RKH_DUO_THRESHOLD, read at create (dynamic space)
  int D = 0, DP = 0;
  uint32_t P = 0, kmax = 0, emax = 0;
  std::vector<GbProblem> prob;
  static constexpr size_t kKnnWsBytes = kKnnBatchWsBytes;  // knn_plan.h: holds every plan of one query
  // command block: [KnnArgs x P][EdgeIO x P][EdgeIO (stage A) x P][GbAux x P], pinned host copy + device copy
  PinnedBuffer<unsigned char> h_cmd;
  DeviceBuffer<unsigned char> d_cmd;
  size_t cmd_bytes = 0;
  KnnArgs *h_knn = nullptr, *d_knn = nullptr;
  EdgeIO *h_io = nullptr, *d_io = nullptr;
  EdgeIO *h_ioa = nullptr, *d_ioa = nullptr;
  GbAux *h_aux = nullptr, *d_aux = nullptr;
  // result block per problem: {kcnt, overflow, n_edges, sel} kidx[kmax] kdist[kmax] nchk[emax] accept[emax] x_out[emax][D]
  //                           a_nchk[16] a_accept[16] a_xout[16][D]
  PinnedBuffer<unsigned char> h_res;
  DeviceBuffer<unsigned char> d_res;
  unsigned char* h_res_dev = nullptr;            // h_res as the device sees it
  PinnedBuffer<uint32_t> h_flag;                 // the step word the host spins on (run())
  uint32_t* h_flag_dev = nullptr;
  DeviceBuffer<uint32_t> d_arrivals;
  uint32_t flag_seq = 0;
  size_t res_stride = 0, off_kidx = 0, off_kdist = 0, off_nchk = 0, off_accept = 0, off_xout = 0, off_anchk = 0,
         off_aaccept = 0, off_axout = 0;
  bool any_knn = false, any_edges = false, any_append = false, any_stage_a = false;
  uint64_t steps = 0;
  uint32_t knn_list_cap = 0;  // RKH_KNN_LIST_CAP at init (rkh_diag.h): shorter candidate lists, same results
  std::vector<uint32_t> knn_k;       // per problem: k, n and radius of the last cmd_knn
  std::vector<uint64_t> knn_n;
  std::vector<double> knn_radius;
  std::vector<double> inf_row;

  // the steerable dynamic free space: vertices are states (q, qd), edges steer_position_toward (planner.hip's space)
  rkh_status init_dynamic(rkh_scene* sc, const rkh_dyn_space* space, uint32_t n_problems, const uint64_t* capacities,
                          uint32_t kmax_);
  rkh_status init(rkh_scene* sc, const rkh_qs_space* space, uint32_t n_problems, const uint64_t* capacities,
                  uint32_t kmax_);
  rkh_status init_common(rkh_scene* sc, int D_, uint32_t n_problems, const uint64_t* capacities, uint32_t kmax_);
  ~GraphBatch();  // waits for the stream and destroys it; the buffers then free themselves

  unsigned char* dres(uint32_t i) const { return d_res.get() + size_t(i) * res_stride; }
  const unsigned char* hres(uint32_t i) const { return h_res.get() + size_t(i) * res_stride; }
  // ---- results of the last run()
  uint32_t kcnt(uint32_t i) const { return reinterpret_cast<const uint32_t*>(hres(i))[0]; }
  uint32_t overflow(uint32_t i) const { return reinterpret_cast<const uint32_t*>(hres(i))[1]; }
  uint32_t n_edges(uint32_t i) const { return reinterpret_cast<const uint32_t*>(hres(i))[2]; }
  const uint32_t* kidx(uint32_t i) const { return reinterpret_cast<const uint32_t*>(hres(i) + off_kidx); }
  const double* kdist(uint32_t i) const { return reinterpret_cast<const double*>(hres(i) + off_kdist); }
  const uint8_t* accept(uint32_t i) const { return hres(i) + off_accept; }
  const double* x_out(uint32_t i) const { return reinterpret_cast<const double*>(hres(i) + off_xout); }
  uint32_t selected(uint32_t i) const { return reinterpret_cast<const uint32_t*>(hres(i))[3]; }
  const double* a_x_out(uint32_t i) const { return reinterpret_cast<const double*>(hres(i) + off_axout); }

  // The neighbourhood of the last cmd_knn of problem i, in the order the reference's search returns it.
  // min_dist_linear_search (topological_search.hpp:244-274) keeps a bounded max-heap ordered by distance alone, so among
  // exactly equal distances both the order of the result and -- when a tie straddles the k-th place -- its members are
  // decided by the heap's history (std::push_heap / pop_heap / sort_heap), while the device returns ascending
  // (distance, index).  Equal distances only arise from coincident vertices (the bidirectional RRT* pulls the same
  // point from both trees at a joining vertex); then, and only then, the search is replayed here on the host copy of
  // the positions with the reference's own sequence of heap operations.  id[e] = vertex, slot[e] = where its edge
  // verdicts sit in accept() / x_out() (a vertex the device did not list borrows the slot of a listed vertex at the
  // same position: its walks are the same walks); the second direction of a GB_LIST_KNN_BIDIR list is at stride + slot.
  struct Neighbours {
    uint32_t K = 0, stride = 0;
    std::vector<uint32_t> id, slot;
  };
  rkh_status neighbours(uint32_t i, const double* host_pos, const double* query, Neighbours* out,
                        const uint8_t* removed = nullptr);

  // the neighbourhood with its edge verdicts gathered in the reference's order: accept[e] / x_out[e] belong to the first
  // direction of neighbour id[e], accept[K + e] / x_out[K + e] to the second one of a GB_LIST_KNN_BIDIR list
  struct Verdicts {
    uint32_t K = 0;
    std::vector<uint32_t> id;
    std::vector<uint8_t> accept;
    std::vector<double> x_out;
  };
  rkh_status verdicts(uint32_t i, const double* host_pos, const double* query, Verdicts* out,
                      const uint8_t* removed = nullptr);

  // ---- command building
  void begin();
  // Stage A: `count` candidates of problem i, tested before this step's k-NN.
  //   GB_SELECT_POINT: is_free(pts[c]);  GB_SELECT_WALK: walk from vertex v towards pts[c] by frac[c], accepted if
  //   the distance travelled exceeds tol * target_dist[c] (random_walk).  The first accepted candidate (point, or
  //   end point of the walk) becomes the query of cmd_knn and is appended as vertex row n_dev.  The caller fills
  //   h_aux[i].pts / frac / target_dist and calls confirm_selected() after run() if selected(i) is valid.
  rkh_status cmd_stage_a(uint32_t i, uint32_t select_mode, uint32_t count, uint32_t v, double tol);
  void confirm_selected(uint32_t i) { ++prob[i].n_dev; }
  // any_knn_synchro::removed_vertex: the row keeps its index and is overwritten with +inf (no sweep returns it);
  // stream-ordered before the next step's kernels
  rkh_status remove_row(uint32_t i, uint32_t row);
  // vertex row n_dev of problem i (the caller's vertex ids are row numbers)
  rkh_status cmd_append(uint32_t i, const double* row);
  // k nearest of `query` among the first n rows, strictly inside `radius`
  rkh_status cmd_knn(uint32_t i, const double* query, uint64_t n, uint32_t k, double radius);
  // candidate edges of this step (see GbListMode); mode / tol as in EdgeIO
  void cmd_edges(uint32_t i, uint32_t list_mode, uint32_t v, int mode, double tol);

  // the steer mapping of a step's launch of up to `edges` edges per problem: one wave per edge, or two
  // (state_derivative_duo) while even that bound leaves half the SIMDs idle (steer_mapping)
  SteerMapping steer(uint32_t edges) const;

  // one device step: command upload, the launches the commands ask for, result download
  rkh_status run();
  // run()'s part behind the k-NN search (it runs a second time after an exact k-NN retry), and whether a search of the
  // results just downloaded overflowed its candidate list
  rkh_status run_after_knn();
  bool knn_overflowed() const;
};

}  // namespace rkh
