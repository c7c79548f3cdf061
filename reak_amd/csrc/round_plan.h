// round_plan.h -- the rules a round of the speculative-batch RRT driver (planner.hip) is planned by, each stated once:
// the batch rule (how many candidates a problem takes), the wave fit (the batch scale that fills whole passes of steer
// waves) and the steer launch plan of an Auto round (which form runs a round of a given edge count).
//
// round_begin_kernel chooses the batches on the device; the host sizes every grid of the round from the same rule at its
// own upper bounds, and launches the steer forms the plan lists.  The rules use no device builtin and no HIP header, so a
// host compiler and a sanitizer can read them on a machine without a GPU (tests/cpp/round_plan_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "round_carry.h"  // RKH_HD, kCarryOff, carry_round

namespace rkh {

// ---- the batch rule ---------------------------------------------------------------------------------------------------
// B = scale * batch_factor * sqrt(n), cut to whole steer waves, clamped to [b_min, b_cap].  Results do not depend on it.
struct BatchInputs {
  float batch_factor;
  float sqrt_n;    // sqrtf(float(vertices))
  uint32_t b_min;  // 0 for a finished problem
  uint32_t b_cap;  // min(b_max, samples available); 0 for a finished problem
};

// epw: edges per steer wave; from epw candidates up a batch is a whole number of waves (0 or 1: no rounding).
// The product is evaluated in this order, in float, and truncated: monotone in scale and in sqrt_n, so the value at an
// upper bound of both (and of b_cap) is an upper bound of the value -- what the host sizes the round's grids by.
RKH_HD uint32_t round_batch(const BatchInputs& in, float scale, uint32_t epw) {
  const float want = scale * in.batch_factor * in.sqrt_n;
  uint32_t B = uint32_t(want);
  if (epw > 1u && B >= epw) B -= B % epw;  // whole steer waves: no half-empty last wave per problem
  if (B < in.b_min) B = in.b_min;
  if (B > in.b_cap) B = in.b_cap;
  return B;
}

// ---- the probe list's granule rule ------------------------------------------------------------------------------------
// A problem's open goal probes (the vertices probe_certified, probe_reach.h, did not settle at commit) wait in a list, in
// vertex order.  A commit first drops the entries the round's launch ran from the front, keeps what that launch left
// behind -- `waited` entries, fewer than the granule -- and appends the round's open vertices behind them: list_n in all.
// The next launch takes the list's whole granules (a (problem, probes) segment of the steer grid then has no half-empty
// last wave), but at least the entries that have waited one round already: open probes are rare, and a waiting one holds
// back probed_n and with it the sync's gather.  What stays behind is again fewer than the granule; granule 1: all ride.
RKH_HD uint32_t probe_ride_count(uint32_t list_n, uint32_t waited, uint32_t granule) {
  const uint32_t whole = granule > 1u ? list_n - list_n % granule : list_n;
  return whole > waited ? whole : waited;
}
// vertices [1, probed_n) have their goal-probe result: up to the first vertex still in the list, else all n
RKH_HD uint32_t probe_probed_n(const uint32_t* list, uint32_t list_n, uint32_t n) { return list_n ? list[0] : n; }

// steer waves (or query blocks) that `count` edges (queries) of one segment take
RKH_HD uint32_t round_waves(uint32_t count, uint32_t epw) { return (count + epw - 1u) / epw; }

// ---- the wave fit -----------------------------------------------------------------------------------------------------
// The two-lanes steer kernel runs `slots` waves at a time, so the steer time of a round is its number of waves over
// `slots`, rounded UP.  The scale is bisected so that the round's waves fill `fill` of a whole number of such passes.
constexpr float kFitScaleLo = 0.75f, kFitScaleHi = 1.4f;  // the host sizes the launches of a fitted round for kFitScaleHi
constexpr float kFitEntryFill = 0.75f;  // a round of at most this share of one pass keeps scale 1
constexpr float kFitPassRound = 0.15f;  // a round up to this far beyond a whole number of passes is fitted down to it
constexpr int kFitSteps = 10;

// waves the round at scale 1 (w1 of them) is fitted to
RKH_HD float fit_target_waves(float w1, uint32_t slots, float fill) {
  const float passes = ceilf(w1 / float(slots) - kFitPassRound);
  return passes * float(slots) * fill;
}

// waves_at(scale): the round's waves at that scale, monotone.  Returns 1 or a scale in [kFitScaleLo, kFitScaleHi) with
// waves_at(scale) <= target wherever waves_at(kFitScaleLo) is.  On the device every thread of the block calls it with
// the same arguments (waves_at is a block-wide sum).
template <class WavesAt>
RKH_HD float fit_batch_scale(const WavesAt& waves_at, uint32_t slots, float fill) {
  const float w1 = float(waves_at(1.0f));
  if (!(w1 > kFitEntryFill * float(slots))) return 1.0f;
  const float target = fit_target_waves(w1, slots, fill);
  float lo = kFitScaleLo, hi = kFitScaleHi;
  for (int it = 0; it < kFitSteps; ++it) {
    const float mid = 0.5f * (lo + hi);
    if (float(waves_at(mid)) > target) hi = mid;
    else lo = mid;
  }
  return lo;
}

// ---- the steer launch plan of an Auto round ---------------------------------------------------------------------------
// Every launch of the plan is enqueued; on the device each compares the round's edge count with its gate [lo, hi) and the
// ones not chosen exit at once.  Small rounds run a form made for latency, large ones the two-lanes form (32 edges per
// wave), step-wise -- one launch per RK4 step over the live edges -- where the round is large enough to gain from it.
enum class SteerForm : uint8_t {
  TwoWaves,   // two waves per edge
  OneWave,    // one wave per edge (chains with prismatic joints: their one-wave form)
  LanesWhole, // two lanes per edge, one launch for the whole edge
  LanesSteps, // two lanes per edge, one launch per RK4 step
};

struct SteerPlanInputs {
  uint32_t lane_threshold = 0;   // rounds of at least this many edges take the two-lanes form
  uint32_t duo_threshold = 0;    // rounds below this many take two waves per edge (0: never)
  uint32_t split_min_edges = 0;  // rounds of at least this many take the step-wise launches
  uint32_t carry_min_edges = kCarryOff;  // step-wise rounds of at least this many carry (round_carry.h); kCarryOff: none
  bool compact = false;    // a regular round, over the segments round_begin_kernel counted (not the probe flush)
  bool stepwise = false;   // the step-wise form exists: more than one RK4 step, its counters are allocated
  bool prismatic = false;  // the chain has prismatic joints: no two-waves form
  uint64_t edges_ub = 0;   // host-side bound on the edges of the round: a launch no round can reach is left out
};

constexpr uint32_t kGateOpenEnd = 0xFFFFFFFFu;
struct SteerLaunch {
  SteerForm form;
  uint32_t lo, hi;  // the gate: lo <= edges < hi
};

struct SteerPlan {
  SteerPlanInputs in;     // what the plan was made from
  SteerLaunch launch[4] = {};  // in ascending order of their gates
  uint32_t n = 0;
  bool restore = false;   // carry_restore_kernel runs in front of the step-wise launch
  uint32_t carry_lo = kCarryOff;  // the fewest edges of a round that carries: carry_round(c, the step-wise gate,
                                  // carry_min_edges) == (c >= carry_lo && c < that gate's hi); kCarryOff: no round does
};

RKH_HD SteerPlan steer_plan(const SteerPlanInputs& in) {
  SteerPlan pl;
  pl.in = in;
  auto add = [&](SteerForm f, uint32_t lo, uint32_t hi) { pl.launch[pl.n++] = SteerLaunch{f, lo, hi}; };
  const uint32_t lane = in.lane_threshold;
  // below the lane threshold: latency.  The smallest rounds (at most half the chip's SIMDs at one wave per edge: a single
  // problem, a few young trees) run two waves per edge -- the f-eval's critical path instead of its instruction count.
  uint32_t wave_lo = 0;
  if (in.duo_threshold > 0 && in.compact && !in.prismatic) {
    wave_lo = in.duo_threshold < lane ? in.duo_threshold : lane;
    add(SteerForm::TwoWaves, 0u, wave_lo);
  }
  if (wave_lo < lane) add(SteerForm::OneWave, wave_lo, lane);
  // from there on: two lanes per edge.  Half of the edges of a round end within a few steps and leave their lanes idle for
  // the rest of their wave, so one launch per step carries only the live edges, in fewer waves -- when the round is large
  // enough; below split_min_edges the extra launches and tails cost more than the idle lanes.
  if (!(in.compact && in.stepwise)) {
    add(SteerForm::LanesWhole, lane, kGateOpenEnd);
    return pl;
  }
  const uint32_t steps_lo = in.split_min_edges > lane ? in.split_min_edges : lane;
  if (in.carry_min_edges != kCarryOff) pl.carry_lo = in.carry_min_edges > steps_lo ? in.carry_min_edges : steps_lo;
  if (steps_lo > lane && in.edges_ub >= lane) add(SteerForm::LanesWhole, lane, steps_lo);
  if (in.edges_ub >= steps_lo) {
    add(SteerForm::LanesSteps, steps_lo, kGateOpenEnd);
    pl.restore = in.carry_min_edges != kCarryOff && in.edges_ub >= in.carry_min_edges;
  }
  return pl;
}

}  // namespace rkh
