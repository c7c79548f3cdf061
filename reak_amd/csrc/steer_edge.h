// steer_edge.h -- the protocol of one candidate edge, each rule once: which rows an edge reads, how many steps it takes,
// the input it holds, the RK4 stage update, the bounds test, and the verdict it leaves (accept byte / goal-probe distance).
// The one-wave steer kernel, the planar kernel and the two edge walks (propagate.hip, propagate_planar.hip) take all of it
// from here; the two two-lanes kernels (propagate_pair.hip) take their verdict from here and keep the rest in their own
// text.  What stays with a kernel is how its grid finds an edge and how it sums the three norms.
//
// The rules use no device builtin and no HIP header, so a host compiler and a sanitizer can read them on a machine
// without a GPU (tests/cpp/steer_edge_test.cpp).  Products, sums and comparisons are written in the reference's order
// (the kernels are compiled with -ffp-contract=off).  Reference paths are relative to src/ReaK/.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define RKH_HD __host__ __device__ __forceinline__
#else
#define RKH_HD inline
#endif

namespace rkh {

constexpr int kMaxSteps = 64;  // RK4 steps per edge

enum EdgeMode : int {
  EDGE_PLAIN = 0,
  EDGE_STEER_ACCEPT = 1,
  EDGE_GOAL_PROBE = 2,
  EDGE_CONNECT = 3,
  EDGE_WALK_ACCEPT = 4,  // random_walk: traveled > steer_tol * best_case[e] (best_case carries the target distance)
  EDGE_STEER_BOTH = 6,   // quasi-static kernel: EDGE_STEER_ACCEPT in bit 0 of accept, bit 1 = the walk ran to its end
  EDGE_POINT = 5,        // accept = is_free(target point), no walk (quasi-static kernel, one-wave-per-edge dynamics kernel)
};

struct EdgeIO {  // inputs / outputs of one propagate launch (all device pointers)
  const double* src = nullptr;         // source rows
  const uint32_t* src_idx = nullptr;   // row of edge e (null: *d_src_first + e, or e)
  const uint32_t* d_src_first = nullptr;
  uint32_t src_stride = 0;
  const double* tgt = nullptr;         // target rows
  const uint32_t* d_tgt_off = nullptr; // row offset read on the device
  const uint32_t* tgt_idx = nullptr;   // optional: target row of edge e (graph planners)
  uint32_t tgt_stride = 0;             // 0: one target for all edges
  const double* frac = nullptr;        // optional per-edge travel fraction (quasi-static kernel; null: QsDev::fraction)
  uint32_t B = 0;
  const uint32_t* d_B = nullptr;
  double* x_out = nullptr;
  uint32_t* steps_free = nullptr;
  double* record = nullptr;
  int record_stride = 0;
  int mode = EDGE_PLAIN;
  const double* best_case = nullptr;
  double steer_tol = 0.1;
  uint8_t* accept = nullptr;
  double* goal_dist = nullptr;         // indexed by source row - 1
  int* err_flag = nullptr;
};

// A steer kernel with a gate runs only if lo <= *count < hi (read on the device); count == nullptr: always.
struct KernelGate {
  const uint32_t* count = nullptr;
  uint32_t lo = 0, hi = 0xFFFFFFFFu;
  // two-lanes kernel, table launches: exclusive prefix of the working waves per segment (segment 2p = candidates of
  // problem p, 2p+1 = its goal probes; wave_base[n_segments] = total).  The blocks of the grid, in dispatch order, then
  // take the working waves one after the other, so the round-robin of blocks over the 8 XCDs spreads the work evenly
  // whatever the per-problem counts are (a (wave, problem) grid leaves holes that land unevenly on the XCDs).
  const uint32_t* wave_base = nullptr;
  uint32_t n_segments = 0;
  // optional diagnostics: the kernel adds the edge-steps it integrated (steps that began with a live edge, the one that
  // ended it included) -- the executed work of a launch, as opposed to n_steps per launched edge
  unsigned long long* steps_exec = nullptr;
  // two-lanes kernels: skip the proximity test of a step that a carried clearance bound settles (SceneDev::has_clearance
  // scenes only; RKH_STEER_CLEARANCE=0 turns it off), and count [0] += edge-steps settled by the bound, [1] += wave-steps
  // that ran the test (rkh_diag_steer_clearance_counts)
  bool clearance = true;
  unsigned long long* clear_stats = nullptr;
};

// the planner's per-round choice between the kernel mappings: true = this launch does nothing.  `gate` points at the
// KernelGate wherever the kernel keeps it (a by-value copy, or the kernarg segment: then each field is a scalar load).
template <class GateP>
RKH_HD bool steer_gate_closed(GateP gate) {
  if (gate->count) {
    const uint32_t c = *gate->count;
    if (c < gate->lo || c >= gate->hi) return true;
  }
  return false;
}

// The segment that holds entry L of a list laid out by the exclusive prefix of its segments' sizes: the lo with
// prefix[lo] <= L < prefix[lo + 1].  Requires n_segments >= 1, prefix[0] == 0 and L < prefix[n_segments].  The bisection
// keeps prefix[lo] <= L < prefix[hi], so empty segments (equal neighbours in the prefix) are never returned.
template <class PrefixP>
RKH_HD uint32_t segment_of(PrefixP prefix, uint32_t n_segments, uint32_t L) {
  uint32_t lo = 0, hi = n_segments;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (prefix[mid] <= L) lo = mid;
    else hi = mid;
  }
  return lo;
}

// source and target row of edge e
RKH_HD uint32_t edge_source_row(const uint32_t* src_idx, const uint32_t* d_src_first, uint32_t e) {
  return src_idx ? src_idx[e] : ((d_src_first ? *d_src_first : 0u) + e);
}
RKH_HD uint64_t edge_target_row(const uint32_t* tgt_idx, const uint32_t* d_tgt_off, uint32_t e) {
  return tgt_idx ? uint64_t(tgt_idx[e]) : ((d_tgt_off ? uint64_t(*d_tgt_off) : 0ull) + e);
}
RKH_HD uint32_t edge_source_row(const EdgeIO& io, uint32_t e) { return edge_source_row(io.src_idx, io.d_src_first, e); }
RKH_HD uint64_t edge_target_row(const EdgeIO& io, uint32_t e) { return edge_target_row(io.tgt_idx, io.d_tgt_off, e); }

// Steps of an edge with a travel fraction of its own (EdgeIO::frac): the steer loop's comparison
// current_time < fraction * (steps_per_edge * dt), current_time accumulated step by step (MEAQR_topology.hpp:503-565).
RKH_HD int edge_step_count(double frac, double full_time, double dt) {
  const double T_goal = frac * full_time;
  double current_time = 0.0;
  int n_steps = 0;
  while (current_time < T_goal && n_steps < kMaxSteps) {
    current_time += dt;
    ++n_steps;
  }
  return n_steps;
}

// PD law towards the steer target with saturation, held over the step (b: target, x: state; q and its rate)
RKH_HD double pd_input(double kp, double kd, double u_max, double bq, double xq, double bqd, double xqd) {
  double v = kp * (bq - xq) + kd * (bqd - xqd);
  if (v > u_max) v = u_max;
  else if (v < -u_max) v = -u_max;
  return v;
}

// hyperbox_topology::is_in_bounds negated (hyperbox_topology.hpp:178-189); lower > upper: a wrapped coordinate
RKH_HD bool hyperbox_out(double lo, double hi, double x) {
  if (lo < hi) return (x < lo) || (x > hi);
  return (x > lo) || (x < hi);
}

// runge_kutta4_integrate_impl (runge_kutta4_integrator_sys.hpp:53-97), time_step = h, one component.  Each loop iteration
// of the reference evaluates f four times that matter (the prime of :69 or the re-prime of :95, then :82, :86, :92);
// they are the stages 0..3 of a rolled loop in the kernels, which keeps one copy of the dynamics in the instruction
// stream.  dp = f at the current end point xe; w = the start of the inner step.
RKH_HD void rk4_stage(int stage, double h, double dp, double& xe, double& w, double& k1, double& k2, double& k3) {
  if (stage == 0) {
    w = xe;
    k1 = h * dp;
    xe = xe + 0.5 * k1;
  } else if (stage == 1) {
    k2 = h * dp;
    xe = w + 0.5 * k2;
  } else if (stage == 2) {
    k3 = h * dp;
    xe = w + k3;
  } else {
    xe = xe + ((((1.0 / 6.0) * k1 + (2.0 / 6.0) * k2) + (h / 6.0) * dp) - (2.0 / 3.0) * k3);
  }
}

// ---- the verdict.  n_ar = |source - result|, n_ab = |source - target|, n_rb = |result - target| (euclidean, summed left
// to right by the kernel).
constexpr int kNoAccept = -1;  // edge_accept: this mode leaves no accept byte
constexpr int kNoWalk = -1;    // completed_walk of a kernel without a predicate walk (the dynamic steer kernels)

// The accept byte of mode, or kNoAccept (EDGE_PLAIN, EDGE_POINT -- its byte is is_free(target) --, EDGE_GOAL_PROBE,
// EDGE_STEER_BOTH in a kernel without a walk, anything unknown: the kernel writes nothing).
//   EDGE_STEER_ACCEPT  planning_visitor_base::steer_towards_position (planning_visitors.hpp:349-360); best_case null:
//                      the distance to the target
//   EDGE_STEER_BOTH    the same in bit 0; bit 1 = the walk completed.  steer_back_to_position(target, source) walks
//                      the same points (move_position_back_to, interpolated_topologies.hpp:165-191) and returns the
//                      same point unless the walk completes, where it returns the source itself (:185-186): its verdict
//                      is bit 0 && !bit 1
//   EDGE_CONNECT       planning_visitor_base::can_be_connected (planning_visitors.hpp:385-395); steer_tol carries the
//                      connection tolerance
//   EDGE_WALK_ACCEPT   planning_visitor_base::random_walk (planning_visitors.hpp:418-421); best_case carries the target
//                      distance
RKH_HD int edge_accept(int mode, double n_ar, double n_ab, double n_rb, const double* best_case, uint32_t e,
                       double steer_tol, int completed_walk) {
  if (mode == EDGE_STEER_ACCEPT || (mode == EDGE_STEER_BOTH && completed_walk != kNoWalk)) {
    const double bc = best_case ? best_case[e] : n_ab;
    const bool ok = (!std::isinf(n_ar)) && (n_ar < 2.0 * bc) && (n_ar > steer_tol * bc);
    return (ok ? 1 : 0) | ((mode == EDGE_STEER_BOTH && completed_walk == 1) ? 2 : 0);
  }
  if (mode == EDGE_CONNECT) return ((!std::isinf(n_ar)) && (n_rb < steer_tol * n_ar)) ? 1 : 0;
  if (mode == EDGE_WALK_ACCEPT) return ((!std::isinf(n_ar)) && (n_ar > steer_tol * best_case[e])) ? 1 : 0;
  return kNoAccept;
}

// The C_free distance an EDGE_GOAL_PROBE edge leaves in goal_dist.  The two rules differ because the reference's two
// spaces do: a steered trajectory never lands on its target, a straight walk that is not stopped does.
//   steerable (dynamic) space, MEAQR_topology.hpp:995-1003: reached = within 5 % of the whole distance
RKH_HD double goal_probe_steerable(double n_ab, double n_rb) { return (n_ab * 0.05 > n_rb) ? n_ab : INFINITY; }
//   interpolated (quasi-static) topology, interp_topo_get_distance_pred (interpolated_topologies.hpp:193-199)
RKH_HD double goal_probe_interpolated(double n_ab, double n_rb) { return (n_rb < DBL_EPSILON) ? n_ab : INFINITY; }

}  // namespace rkh
