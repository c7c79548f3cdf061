// round_plan_test.cpp -- host-only check of the rules a planner round is planned by (reak_amd/csrc/round_plan.h): the
// batch rule and the host's bound of it, the wave fit, the steer launch plan of an Auto round.  Built with
// -fsanitize=address,undefined and run directly (tests/test_round_plan_cpu.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "round_plan.h"

using namespace rkh;

static int g_checks = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// ---- the batch rule ---------------------------------------------------------------------------------------------------
// what round_begin_kernel loads for a problem of n vertices with `avail` samples left (planner.hip: batch_inputs)
static BatchInputs device_inputs(float bf, uint32_t n, uint32_t b_min, uint32_t b_max, uint32_t avail, bool done) {
  return BatchInputs{bf, sqrtf(float(n)), done ? 0u : b_min, done ? 0u : (b_max < avail ? b_max : avail)};
}
// what the host sizes the round's grids by (planner.hip: batch_upper_bound): its vertex bound, no availability clamp
static uint32_t host_bound(float bf, uint64_t n_ub, uint32_t b_min, uint32_t b_max, float scale) {
  return round_batch(BatchInputs{bf, sqrtf(float(n_ub)), b_min, b_max}, scale, 1u);
}

static void batch_tests() {
  std::vector<uint32_t> ns;
  for (uint32_t n = 1; n <= 4096; ++n) ns.push_back(n);
  for (uint32_t k = 13; k <= 24; ++k)
    for (uint32_t n : {(1u << k) - 1u, 1u << k, (1u << k) + 1u}) ns.push_back(n);
  // scales of the named range: its ends, the last float below the upper end, the first mids of the bisection
  const float scales[] = {kFitScaleLo, 0.9f, 1.0f, 0.5f * (kFitScaleLo + kFitScaleHi), 1.2375f, 1.39f,
                          nextafterf(kFitScaleHi, 0.0f), kFitScaleHi};
  for (float bf : {1.25f, 2.0f, 4.0f})
    for (uint32_t b_min : {1u, 8u})
      for (uint32_t b_max : {8u, 384u, 1024u, 4096u})
        for (uint32_t epw : {1u, 32u})
          for (uint32_t n : ns) {
            // the host's bound at the vertex bounds a sync and the enqueued rounds leave it with
            uint32_t ub_fit = 0xFFFFFFFFu, ub_one = 0xFFFFFFFFu;
            for (uint64_t n_ub : {uint64_t(n), uint64_t(n) + 1u, uint64_t(n) + b_max, 2u * uint64_t(n)}) {
              const uint32_t f = host_bound(bf, n_ub, b_min, b_max, kFitScaleHi), o = host_bound(bf, n_ub, b_min, b_max, 1.0f);
              CHECK(f >= o);
              ub_fit = f < ub_fit ? f : ub_fit;
              ub_one = o < ub_one ? o : ub_one;
            }
            CHECK(ub_fit >= b_min || b_min > b_max);
            CHECK(ub_fit <= b_max);
            for (uint32_t avail : {0u, 1u, 31u, 32u, 33u, b_max - 1u, b_max, b_max + 1u, 0x7FFFFFFFu}) {
              for (float sc : scales) {  // the wave fit is on: any scale of the range, whole waves
                const uint32_t B = round_batch(device_inputs(bf, n, b_min, b_max, avail, false), sc, epw);
                CHECK(B <= ub_fit);
                CHECK(B <= avail && B <= b_max);
                CHECK(B >= b_min || B == avail || B == b_max);
                CHECK(round_waves(B, 32u) * 32u >= B && round_waves(B, 32u) * 32u < B + 32u);
              }
              // the wave fit is off: scale 1 on both sides, no rounding
              CHECK(round_batch(device_inputs(bf, n, b_min, b_max, avail, false), 1.0f, 1u) <= ub_one);
              CHECK(round_batch(device_inputs(bf, n, b_min, b_max, avail, true), kFitScaleHi, epw) == 0u);
            }
          }
  // the edges, pinned.  Wave rounding applies from epw candidates up ...
  const uint32_t big = 4096u;
  CHECK(round_batch(BatchInputs{1.0f, 31.5f, 1u, big}, 1.0f, 32u) == 31u);
  CHECK(round_batch(BatchInputs{1.0f, 32.0f, 1u, big}, 1.0f, 32u) == 32u);
  CHECK(round_batch(BatchInputs{1.0f, 33.9f, 1u, big}, 1.0f, 32u) == 32u);
  CHECK(round_batch(BatchInputs{1.0f, 63.9f, 1u, big}, 1.0f, 32u) == 32u);
  CHECK(round_batch(BatchInputs{1.0f, 64.0f, 1u, big}, 1.0f, 32u) == 64u);
  CHECK(round_batch(BatchInputs{2.0f, 20.0f, 1u, big}, 1.25f, 32u) == 32u);  // 50 -> 32
  // ... and not without a granule
  CHECK(round_batch(BatchInputs{1.0f, 33.9f, 1u, big}, 1.0f, 1u) == 33u && round_batch(BatchInputs{1.0f, 33.9f, 1u, big}, 1.0f, 0u) == 33u);
  // b_min above the wave-rounded value: the lower clamp comes after the rounding
  CHECK(round_batch(BatchInputs{1.0f, 40.0f, 36u, big}, 1.0f, 32u) == 36u);
  CHECK(round_batch(BatchInputs{1.0f, 2.0f, 8u, big}, 1.0f, 32u) == 8u);
  // the upper clamp last: b_max, what is left of the sample stream, nothing left, a finished problem
  CHECK(round_batch(BatchInputs{4.0f, 1000.0f, 8u, 384u}, 1.4f, 32u) == 384u);
  CHECK(round_batch(device_inputs(1.25f, 10000u, 8u, 1024u, 5u, false), 1.0f, 32u) == 5u);
  CHECK(round_batch(device_inputs(1.25f, 10000u, 8u, 1024u, 0u, false), 1.0f, 32u) == 0u);
  CHECK(round_batch(device_inputs(1.25f, 10000u, 8u, 1024u, 5000u, true), 1.0f, 32u) == 0u);
  // the float product, truncated: 1.25 sqrt(n) reaches 384 at n = 94372 (307.2 ^ 2 = 94371.84)
  CHECK(round_batch(device_inputs(1.25f, 94372u, 8u, 4096u, 5000u, false), 1.0f, 1u) == 384u);
  CHECK(round_batch(device_inputs(1.25f, 94371u, 8u, 4096u, 5000u, false), 1.0f, 1u) == 383u);
  CHECK(round_waves(0u, 32u) == 0u && round_waves(1u, 32u) == 1u && round_waves(32u, 32u) == 1u && round_waves(33u, 32u) == 2u);
}

// ---- the wave fit -----------------------------------------------------------------------------------------------------
static void fit_tests() {
  for (uint32_t slots : {1024u, 2048u})
    for (float fill : {0.99f, 0.9f}) {
      // linear: `full` waves at scale 1
      for (uint32_t full = 0; full <= 6u * slots; full += 37u) {
        int calls = 0;
        auto waves_at = [&](float sc) {
          ++calls;
          return uint32_t(sc * float(full));
        };
        const float sc = fit_batch_scale(waves_at, slots, fill);
        if (float(full) <= kFitEntryFill * float(slots)) {  // a round that does not fill a pass keeps its batches
          CHECK(sc == 1.0f && calls == 1);
          continue;
        }
        CHECK(calls == 1 + kFitSteps);
        CHECK(sc >= kFitScaleLo && sc < kFitScaleHi);
        const float target = fit_target_waves(float(full), slots, fill);
        CHECK(float(waves_at(sc)) <= target);
        // the bisection's answer: no scale two of its last steps further up fits, unless the upper end does
        CHECK(float(waves_at(sc + (kFitScaleHi - kFitScaleLo) / 512.0f)) > target || float(waves_at(kFitScaleHi)) <= target);
      }
      // steps: P problems of b candidates at scale 1, whole 32-edge waves each, plus one probe wave each
      for (uint32_t P : {1u, 256u, 1025u})
        for (uint32_t b : {8u, 100u, 384u}) {
          auto waves_at = [&](float s) { return P * (round_waves(round_batch(BatchInputs{1.0f, float(b), 8u, 4096u}, s, 32u), 32u) + 1u); };
          const float sc = fit_batch_scale(waves_at, slots, fill);
          const float w1 = float(waves_at(1.0f));
          if (w1 <= kFitEntryFill * float(slots)) {
            CHECK(sc == 1.0f);
            continue;
          }
          CHECK(sc >= kFitScaleLo && sc < kFitScaleHi);
          CHECK(float(waves_at(sc)) <= fit_target_waves(w1, slots, fill) || float(waves_at(kFitScaleLo)) > fit_target_waves(w1, slots, fill));
        }
    }
  CHECK(fit_target_waves(1100.0f, 1024u, 0.99f) == 1.0f * 1024.0f * 0.99f);  // 1.07 passes: fitted down to one
  CHECK(fit_target_waves(1200.0f, 1024u, 0.99f) == 2.0f * 1024.0f * 0.99f);  // 1.17 passes: up to two
}

// ---- the steer launch plan --------------------------------------------------------------------------------------------
static int gates_open(const SteerPlan& pl, uint32_t c) {
  int n = 0;
  for (uint32_t k = 0; k < pl.n; ++k) n += (c >= pl.launch[k].lo && c < pl.launch[k].hi) ? 1 : 0;
  return n;
}
static const SteerLaunch* find(const SteerPlan& pl, SteerForm f, int nth = 0) {
  for (uint32_t k = 0; k < pl.n; ++k)
    if (pl.launch[k].form == f && nth-- == 0) return &pl.launch[k];
  return nullptr;
}
static bool same(const SteerLaunch& l, SteerForm f, uint32_t lo, uint32_t hi) { return l.form == f && l.lo == lo && l.hi == hi; }

static void plan_tests() {
  const uint32_t lanes[] = {0u, 1u, 1024u}, duos[] = {0u, 512u, 1024u, 4096u}, splits[] = {0u, 1024u, 32768u, 1000000000u};
  const uint32_t carries[] = {kCarryOff, 0u, 32768u};
  const uint64_t ubs[] = {0u, 1u, 1023u, 1024u, 32767u, 32768u, 1000000u};
  for (uint32_t lane : lanes)
    for (uint32_t duo : duos)
      for (uint32_t split : splits)
        for (uint32_t carry_min : carries)
          for (int flags = 0; flags < 8; ++flags)
            for (uint64_t ub : ubs) {
              SteerPlanInputs in;
              in.lane_threshold = lane;
              in.duo_threshold = duo;
              in.split_min_edges = split;
              in.carry_min_edges = carry_min;
              in.compact = (flags & 1) != 0;
              in.stepwise = (flags & 2) != 0;
              in.prismatic = (flags & 4) != 0;
              in.edges_ub = ub;
              const SteerPlan pl = steer_plan(in);
              CHECK(pl.n >= 1 || ub < lane);
              CHECK(pl.n <= 4);
              // ascending, pairwise disjoint
              for (uint32_t k = 0; k < pl.n; ++k) {
                CHECK(pl.launch[k].lo <= pl.launch[k].hi);
                if (k) CHECK(pl.launch[k - 1].hi <= pl.launch[k].lo);
              }
              // every count a round can have opens exactly one gate; one it cannot have opens at most one, and none only
              // where the launch was left out as unreachable
              std::vector<uint32_t> counts = {0u, 1u, 2u, 511u, 512u, 513u, 1023u, 1024u, 1025u, 4095u, 4096u, 32767u, 32768u,
                                              32769u, 999999u, 1000000u, 1000001u, 999999999u, 1000000000u, 0xFFFFFFFEu};
              counts.push_back(uint32_t(ub));
              counts.push_back(uint32_t(ub) + 1u);
              for (uint32_t c : counts) {
                const int open = gates_open(pl, c);
                CHECK(open <= 1);
                CHECK(open == 1 || c > ub);
              }
              const SteerLaunch* two = find(pl, SteerForm::TwoWaves);
              const SteerLaunch* one = find(pl, SteerForm::OneWave);
              const SteerLaunch* steps = find(pl, SteerForm::LanesSteps);
              CHECK(!two || (!in.prismatic && in.compact && duo > 0));
              CHECK(!one || one->lo < one->hi);  // an empty one-wave interval is not launched
              CHECK(!steps || (in.stepwise && in.compact));
              CHECK(!find(pl, SteerForm::TwoWaves, 1) && !find(pl, SteerForm::OneWave, 1) && !find(pl, SteerForm::LanesSteps, 1));
              // rounds that are not regular ones: one whole-edge two-lanes launch from the lane threshold up
              if (!(in.compact && in.stepwise)) {
                CHECK(pl.n >= 1 && same(pl.launch[pl.n - 1], SteerForm::LanesWhole, lane, kGateOpenEnd));
              }
              const bool carry_on = carry_min != kCarryOff;
              CHECK(pl.restore == (steps && carry_on && ub >= carry_min));
              if (steps) {
                CHECK(steps->hi == kGateOpenEnd && steps->lo == (split > lane ? split : lane));
                for (uint32_t c : counts)
                  CHECK(carry_round(c, steps->lo, steps->hi, carry_min) == (c >= pl.carry_lo && c < steps->hi));
              } else {
                CHECK(pl.carry_lo == kCarryOff || pl.carry_lo > ub);  // no round reaches it
              }
              CHECK(carry_on || pl.carry_lo == kCarryOff);
            }
  // The default configuration: 256 CUs at two waves per SIMD are 2048 resident steer waves, split = carry = 1024 x 32.
  {
    SteerPlanInputs in;
    in.lane_threshold = 1024u;
    in.duo_threshold = 512u;
    in.split_min_edges = in.carry_min_edges = 32768u;
    in.compact = in.stepwise = true;
    in.edges_ub = 256u * (384u + 384u + 32u);
    SteerPlan pl = steer_plan(in);
    CHECK(pl.n == 4 && same(pl.launch[0], SteerForm::TwoWaves, 0u, 512u) && same(pl.launch[1], SteerForm::OneWave, 512u, 1024u) &&
          same(pl.launch[2], SteerForm::LanesWhole, 1024u, 32768u) && same(pl.launch[3], SteerForm::LanesSteps, 32768u, kGateOpenEnd));
    CHECK(pl.restore && pl.carry_lo == 32768u);
    in.edges_ub = 32767u;  // young trees: the step-wise launch cannot be reached
    pl = steer_plan(in);
    CHECK(pl.n == 3 && same(pl.launch[2], SteerForm::LanesWhole, 1024u, 32768u) && !pl.restore && pl.carry_lo == 32768u);
    in.edges_ub = 1023u;  // a single problem: nor can the two-lanes form
    pl = steer_plan(in);
    CHECK(pl.n == 2 && same(pl.launch[0], SteerForm::TwoWaves, 0u, 512u) && same(pl.launch[1], SteerForm::OneWave, 512u, 1024u));
    in.edges_ub = 1000000u;
    in.compact = false;  // the probe flush
    pl = steer_plan(in);
    CHECK(pl.n == 2 && same(pl.launch[0], SteerForm::OneWave, 0u, 1024u) && same(pl.launch[1], SteerForm::LanesWhole, 1024u, kGateOpenEnd) &&
          !pl.restore && pl.carry_lo == kCarryOff);
    in.compact = true;
    in.prismatic = true;  // chains with prismatic joints: the one-wave form below the lane threshold
    pl = steer_plan(in);
    CHECK(pl.n == 3 && same(pl.launch[0], SteerForm::OneWave, 0u, 1024u) && same(pl.launch[1], SteerForm::LanesWhole, 1024u, 32768u) &&
          same(pl.launch[2], SteerForm::LanesSteps, 32768u, kGateOpenEnd) && pl.restore && pl.carry_lo == 32768u);
  }
  // The configuration of tests/test_round_carry_gpu.py: RKH_LANE_THRESHOLD=1, split 0, carry from 0 edges.
  {
    SteerPlanInputs in;
    in.lane_threshold = 1u;
    in.duo_threshold = 512u;
    in.split_min_edges = 0u;
    in.carry_min_edges = 0u;
    in.compact = in.stepwise = true;
    in.edges_ub = 3u * (1024u + 1024u + 32u);
    const SteerPlan pl = steer_plan(in);
    CHECK(pl.n == 2 && same(pl.launch[0], SteerForm::TwoWaves, 0u, 1u) && same(pl.launch[1], SteerForm::LanesSteps, 1u, kGateOpenEnd));
    CHECK(pl.restore && pl.carry_lo == 1u);
  }
}

int main() {
  batch_tests();
  fit_tests();
  plan_tests();
  std::printf("round plan ok: %d checks\n", g_checks);
  return 0;
}
