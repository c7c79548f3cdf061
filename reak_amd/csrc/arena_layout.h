// arena_layout.h -- where the device buffers of a batch RRT planner (planner.hip) sit inside its one slab.
//
// Plain host C++: no HIP header, no device code, so a host compiler and a sanitizer can read it on a machine without a
// GPU (tests/cpp/arena_layout_test.cpp).  planner_arena_layout is a pure function of the shape of the batch: it hands
// out byte ranges at kArenaAlign, one after the other, and leaves kArenaGuardBytes behind the last one -- buffers that
// ended an allocation of their own had page slack behind them, and a padded-tile read a little past the last range must
// stay inside the slab.  Ranges that a shape does not need (no mirror, no profile, no two-lanes workspace, no carry) have 0 bytes
// and take no room.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rkh {

constexpr size_t kArenaAlign = 256;
constexpr size_t kArenaGuardBytes = 64 * 1024;

constexpr size_t arena_align_up(size_t v) { return (v + kArenaAlign - 1) / kArenaAlign * kArenaAlign; }

struct ArenaRange {
  size_t off = 0, bytes = 0;  // bytes as asked for; the next range starts at arena_align_up(off + bytes)
};

// What all problems share.  The ranges up to SR_UPLOAD_END are filled by ONE host-to-device copy from a pinned block of
// the same layout (the tables, the sampled box, and the zeroes of the round counters and prefixes).
enum SharedRange : int {
  SR_BOUNDS, SR_STATES, SR_PROBS, SR_NN_ARGS, SR_IO_STEER, SR_IO_PROBE, SR_INIT_TAB,
  SR_WAVE_BASE, SR_STEP_CNT, SR_NN_BASE, SR_SEL, SR_STEPS_EXEC,
  SR_UPLOAD_END,
  SR_SAMPLE_TAB0 = SR_UPLOAD_END, SR_SAMPLE_TAB1, SR_GOAL_TAB, SR_LANE_WS, SR_STEP_LIST0, SR_STEP_LIST1,
  SR_COUNT
};
// The 26 buffers of one problem.  PR_STASH_*: what a round's discarded candidates leave for the next one (round_carry.h).
// PR_PROBE_LIST: the vertices whose goal probe is open (round_plan.h, the granule rule: fewer than the granule wait, a
// round appends at most b_max).
enum ProblemRange : int {
  PR_MT, PR_TREE, PR_PARENT, PR_NODE_SAMPLE, PR_GOAL_DIST, PR_SAMPLES, PR_NN_SEQ, PR_ACCEPT_LOG, PR_NN_IDX, PR_NN_DIST,
  PR_X_OUT, PR_STEPS, PR_ACCEPT, PR_PROBE_X, PR_PROBE_STEPS, PR_PROBE_LIST, PR_GOAL, PR_PART_DIST, PR_PART_IDX, PR_ROUND_N,
  PR_MIRROR, PR_CAND, PR_STASH_X, PR_STASH_NN, PR_STASH_STEPS, PR_STASH_ACCEPT,
  PR_COUNT
};

// vertex rows of a problem's tree: max_vertices + the root, in whole 256-row tiles (the NN sweeps)
constexpr uint64_t planner_capacity_rows(uint64_t max_vertices) { return (max_vertices + 1 + 255) / 256 * 256; }
// samples a problem's first stream buffers hold (they grow later, see grow_sample_buffers)
inline uint64_t planner_sample_cap(uint64_t max_vertices, uint32_t b_max, uint64_t cap_min) {
  return std::max<uint64_t>(std::max<uint64_t>(4 * (max_vertices + 1) + 4 * uint64_t(b_max), 1u << 14), cap_min);
}

struct ArenaShape {
  uint32_t P = 0;
  const uint64_t* capacity = nullptr;      // [P] planner_capacity_rows
  const uint64_t* sample_cap = nullptr;    // [P] planner_sample_cap
  const uint64_t* mirror_bytes = nullptr;  // [P] bytes of the tree's half-precision mirror (mirror only)
  uint32_t b_max = 0, probe_granule = 0, part_blocks = 0, prof_rounds = 0;
  int D = 0, DP = 0;
  bool mirror = false, profile = false, lane = false;
  bool carry = false;          // rounds may reuse the discarded candidates of the round before (needs lane)
  size_t cand_bytes = 0;       // per-query scratch of the mirror sweep + the mirror's error word (mirror only)
  size_t lane_ws_bytes = 0;    // workspace of the two-lanes steer kernels (lane only)
  size_t step_list_bytes = 0;  // one of the two lists of the step-wise steer launches (lane only)
  // bytes per entry of the device tables
  size_t state_bytes = 0, prob_bytes = 0, nn_args_bytes = 0, edge_io_bytes = 0, init_bytes = 0, sample_seg_bytes = 0,
         goal_seg_bytes = 0;
  uint32_t max_steps = 0;  // RK4 steps per edge (sizes the step counters)
};

struct ArenaLayout {
  ArenaRange shared[SR_COUNT];
  std::vector<ArenaRange> problem;  // [P][PR_COUNT]
  size_t upload_bytes = 0;          // [0, upload_bytes): the ranges before SR_UPLOAD_END
  size_t total = 0;                 // bytes of the slab, guard tail included
  const ArenaRange& of(uint32_t i, ProblemRange r) const { return problem[size_t(i) * PR_COUNT + r]; }
};

inline ArenaLayout planner_arena_layout(const ArenaShape& s) {
  ArenaLayout L;
  size_t cur = 0;
  auto take = [&cur](size_t bytes) {
    ArenaRange r;
    r.off = cur;
    r.bytes = bytes;
    cur = arena_align_up(cur + bytes);
    return r;
  };
  const size_t P = s.P, b = s.b_max, D = size_t(s.D), DP = size_t(s.DP);
  L.shared[SR_BOUNDS] = take(2 * D * sizeof(double));
  L.shared[SR_STATES] = take(P * s.state_bytes);
  L.shared[SR_PROBS] = take(P * s.prob_bytes);
  L.shared[SR_NN_ARGS] = take(P * s.nn_args_bytes);
  L.shared[SR_IO_STEER] = take(P * s.edge_io_bytes);
  L.shared[SR_IO_PROBE] = take(P * s.edge_io_bytes);
  L.shared[SR_INIT_TAB] = take(P * s.init_bytes);
  // two prefix arrays of 2 P + 1 entries: waves of the two-lanes kernel, then single edges (one-wave-per-edge kernel)
  L.shared[SR_WAVE_BASE] = take(s.lane ? 2 * (2 * P + 1) * sizeof(uint32_t) : 0);
  L.shared[SR_STEP_CNT] = take(s.lane ? 2 * (size_t(s.max_steps) + 1) * sizeof(uint32_t) : 0);
  L.shared[SR_NN_BASE] = take((P + 1) * sizeof(uint32_t));
  L.shared[SR_SEL] = take(2 * sizeof(uint32_t));
  L.shared[SR_STEPS_EXEC] = take(sizeof(unsigned long long));
  L.upload_bytes = cur;
  L.shared[SR_SAMPLE_TAB0] = take(P * s.sample_seg_bytes);
  L.shared[SR_SAMPLE_TAB1] = take(P * s.sample_seg_bytes);
  L.shared[SR_GOAL_TAB] = take(P * s.goal_seg_bytes);
  L.shared[SR_LANE_WS] = take(s.lane ? s.lane_ws_bytes : 0);
  L.shared[SR_STEP_LIST0] = take(s.lane ? s.step_list_bytes : 0);
  L.shared[SR_STEP_LIST1] = take(s.lane ? s.step_list_bytes : 0);
  L.problem.resize(P * PR_COUNT);
  for (size_t i = 0; i < P; ++i) {
    ArenaRange* r = &L.problem[i * PR_COUNT];
    const size_t cap = size_t(s.capacity[i]), scap = size_t(s.sample_cap[i]);
    r[PR_MT] = take((624 + 1) * sizeof(uint32_t));  // mt19937: state words + position
    r[PR_TREE] = take(cap * DP * sizeof(double));
    r[PR_PARENT] = take(cap * sizeof(uint32_t));
    r[PR_NODE_SAMPLE] = take(cap * sizeof(uint32_t));
    r[PR_GOAL_DIST] = take(cap * sizeof(double));
    r[PR_SAMPLES] = take(scap * D * sizeof(double));
    r[PR_NN_SEQ] = take(scap * sizeof(uint32_t));
    r[PR_ACCEPT_LOG] = take(scap);
    r[PR_NN_IDX] = take(b * sizeof(uint32_t));
    r[PR_NN_DIST] = take(b * sizeof(double));
    r[PR_X_OUT] = take(b * D * sizeof(double));
    r[PR_STEPS] = take(b * sizeof(uint32_t));
    r[PR_ACCEPT] = take(b);
    r[PR_PROBE_X] = take((b + s.probe_granule) * D * sizeof(double));
    r[PR_PROBE_STEPS] = take((b + s.probe_granule) * sizeof(uint32_t));
    r[PR_PROBE_LIST] = take((b + s.probe_granule) * sizeof(uint32_t));
    r[PR_GOAL] = take(D * sizeof(double));
    r[PR_PART_DIST] = take(size_t(s.part_blocks) * b * sizeof(double));
    // one more row than the partials need: NnArgs::seed (sampled minima of the matrix-core sweep, "none" = all ones)
    r[PR_PART_IDX] = take((size_t(s.part_blocks) + 1) * b * sizeof(uint32_t));
    r[PR_ROUND_N] = take(s.profile ? 2 * size_t(s.prof_rounds) * sizeof(uint32_t) : 0);
    r[PR_MIRROR] = take(s.mirror ? size_t(s.mirror_bytes[i]) : 0);
    r[PR_CAND] = take(s.mirror ? s.cand_bytes : 0);
    // rows [cut, B) of x_out, nn_idx, steps and accept, packed from slot 0
    const size_t stash = (s.lane && s.carry) ? b : 0;
    r[PR_STASH_X] = take(stash * D * sizeof(double));
    r[PR_STASH_NN] = take(stash * sizeof(uint32_t));
    r[PR_STASH_STEPS] = take(stash * sizeof(uint32_t));
    r[PR_STASH_ACCEPT] = take(stash);
  }
  L.total = cur + kArenaGuardBytes;
  return L;
}

}  // namespace rkh
