// planner.hip -- speculative-batch RRT driver: rrt_planner::solve_planning_query with
// LINEAR_SEARCH_KNN / UNIDIRECTIONAL_PLANNING (ctrl/path_planning/rrt_path_planner.tpp:66-145)
// -> generate_rrt (ctrl/graph_alg/rr_tree.hpp:179-199) over the steerable dynamic space, for a batch of
// P independent planning problems (seeds / queries) on one scene.
//
// generate_rrt is a strict recurrence (sample i's nearest neighbour depends on the vertices added
// by samples < i), but with linear-search NN every RNG draw is a sample coordinate, so the sample
// stream is known in advance.  One round takes, per problem, the next B samples and, against the tree
// snapshot:
//   1. nn1 sweep            (nn_sweep.hip)    nearest snapshot vertex of every sample
//   2. propagate            (propagate.hip)   steer + collision-check all B candidate edges, accept test;
//                                             the same launch runs the open goal probes (edge_added's
//                                             query.get_distance_to_goal) of the previous round's new vertices: those
//                                             the commit could not settle from a travel bound (probe_reach.h)
//   3. fixup  (this file)   candidate b is INVALID iff a vertex that an earlier accepted candidate of the
//                           same round would add is strictly closer to sample b than its snapshot NN
//                           (strict '<' = first-minimum-wins, new vertices have higher indices)
//   4. commit (this file)   everything before the first invalid candidate is exactly what the sequential
//                           algorithm does: append accepted end states in order, log nn/accept per sample
// The next round restarts at the first invalid sample.  Vertex ids, parents, sample consumption and the
// stop condition therefore equal the sequential planner's.  All P problems share each kernel launch
// (blockIdx.y/z = problem) and all per-problem state (vertex count, stream offset, batch size) lives on the
// device, so rounds are enqueued back to back without host round trips and the grids are large enough to fill
// the chip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "arena_layout.h"
#include "nn_device.h"
#include "nn_mirror.h"
#include "probe_reach.h"
#include "rkh_internal.h"
#include "round_carry.h"
#include "round_plan.h"

namespace rkh {

struct PlannerState {  // device-resident, one per problem
  uint32_t n;            // vertices in the tree
  uint32_t s0;           // next sample (== generate_rrt iterations so far)
  uint32_t B;            // candidates of the current round
  uint32_t F;            // first invalid candidate of the current round
  uint32_t list_n;       // open goal probes: entries of ProblemDev::probe_list (vertices probe_certified did not settle)
  uint32_t n_new;        // the first n_new entries of the list ride in the next propagate launch (probe_ride_count)
  uint32_t probed_n;     // vertices [1, probed_n) have their goal probe result in goal_dist
  uint32_t done;         // 1: keep_going() == false (vertex budget reached); 2: sample stream exhausted
  uint32_t max_total;    // max_vertices + 1 (root is not counted by m_iteration_count)
  uint32_t samples_ready;  // samples uploaded so far
  uint32_t b_max;
  float batch_factor;
  uint32_t b_min;
  uint32_t carried;      // candidates the last commit left in the stash (round_carry.h); 0 wherever the stash is not valid
  unsigned long long rounds, edges_speculated, fixup_cut;
  unsigned long long cand_discarded, cand_reused;  // candidates [cut, B) of all rounds; those a later round did not steer again
  unsigned long long probes_certified, probes_run;  // goal probes settled at commit (probe_reach.h); those a steer launch ran
};

struct ProblemDev {  // device pointers of one problem
  PlannerState* st;
  double* tree;
  uint32_t* parent;
  uint32_t* node_sample;
  const double* samples;
  uint32_t* nn_seq;
  uint8_t* accept_log;
  uint32_t* nn_idx;
  double* nn_dist;
  double* x_out;
  uint8_t* accept;
  uint32_t* steps;
  // what the discarded candidates of the last round left (round_carry.h); null: this planner's rounds never carry
  double* stash_x;
  uint32_t* stash_nn;
  uint32_t* stash_steps;
  uint8_t* stash_accept;
  uint32_t* round_n;  // profiling: vertex count at the start of each round (may be null)
  uint4* mirror;      // half-precision mirror of the tree rows (nn_mirror.h), or null
  uint32_t* dx_max_bits;  // its running maximum of |x - x_h|
  double mirror_scale;    // its prescale (mirror_prescale of the planner's coordinate bound)
  // the goal probes: the query's goal state, the results (indexed by vertex - 1), and the list of the open ones in vertex
  // order -- the probe EdgeIO's src_idx ([b_max + kProbeGranule], round_plan.h: the granule rule)
  const double* goal;
  double* goal_dist;
  uint32_t* probe_list;
};

// what commit_kernel settles goal probes by (probe_reach.h); reach_q = +inf: no certificate, every vertex goes to the list
// Only rounds of at least min_edges edges (*round_edges, the count round_begin_kernel summed) settle probes: a smaller
// round runs under one steer wave per SIMD, where its length is that of its longest edge and the probes ride in slots
// that are idle anyway -- the scope of the round carry (round_carry.h), and for its reason: below it every mapping still
// steers the same edges in the same segments, so executed steps and tested wave-steps compare across the mappings.
struct ProbeReachDev {
  double reach_q;
  const uint32_t* round_edges;
  uint32_t min_edges;
  double v_lower[kReachMaxDof], v_upper[kReachMaxDof];  // the velocity bounds of the state box, per joint
};

// round_begin_kernel's arguments (round_begin_args builds them from the planner)
struct RoundBeginArgs {
  const ProblemDev* probs;
  uint32_t P;
  uint32_t round_slot;  // profiling: this round's slot of ProblemDev::round_n
  // sel: {edge counter of even rounds, of odd rounds}.  Every problem adds its candidates + pending goal probes to the
  // counter of this round's parity and block 0 clears the other one for the next round; the steer kernels of the round
  // compare the sum with their gates (steer_plan).
  uint32_t* sel;
  uint32_t parity;
  float fit_fill;   // the wave fit's target fill of the last pass of steer waves; 0: no fit, scale 1
  uint32_t slots;   // concurrent waves of the two-lanes steer kernel
  // exclusive prefixes over the problems, written for the round's compact launch mappings (null: not needed): steer waves
  // per (candidates | probes) segment of the two-lanes kernel, single edges per segment of the one-wave-per-edge kernel,
  // query blocks of nn_queries queries of the NN sweep
  uint32_t* wave_base;  // [2 P + 1]
  uint32_t* edge_base;  // [2 P + 1]
  uint32_t* nn_base;    // [P + 1]
  uint32_t nn_queries;
  uint32_t epw;         // edges per steer wave (pair_kernel_edges_per_wave)
  uint32_t* step_cnt;   // live-edge counters of the step-wise steer launches (two per step: front and back of its list)
  uint32_t carry_fit_lo;  // the fewest edges of a round that carries (SteerPlan::carry_lo); kCarryOff: the fit does not look
};

constexpr uint32_t kProfRounds = 8192;  // profiled rounds per planner (RKH_PROFILE_NN)
constexpr uint32_t kProbeGranule = 32;  // goal probes ride in whole steer waves when the wave fit is on (commit_kernel)

// the batch rule's inputs of a problem as its state stands
__device__ __forceinline__ BatchInputs batch_inputs(const PlannerState* st) {
  const bool done = st->done != 0u;
  const uint32_t avail = st->samples_ready - st->s0;
  BatchInputs in;
  in.batch_factor = st->batch_factor;
  in.sqrt_n = sqrtf(float(st->n));
  in.b_min = done ? 0u : st->b_min;
  in.b_cap = done ? 0u : (st->b_max < avail ? st->b_max : avail);  // the two upper clamps
  return in;
}

// One block for all problems: the batch of every problem (round_plan.h: the batch rule, and with fit_fill > 0 the wave fit
// over the exact counts -- candidates plus the pending goal probes of every problem), the round's edge count, the
// prefixes of the compact launch mappings.
__global__ __launch_bounds__(256) void round_begin_kernel(const RoundBeginArgs args) {
  const ProblemDev* __restrict__ const probs = args.probs;
  uint32_t* __restrict__ const sel = args.sel;
  uint32_t* __restrict__ const wave_base = args.wave_base;
  uint32_t* __restrict__ const edge_base = args.edge_base;
  uint32_t* __restrict__ const nn_base = args.nn_base;
  uint32_t* __restrict__ const step_cnt = args.step_cnt;
  const uint32_t P = args.P, round_slot = args.round_slot, parity = args.parity, slots = args.slots;
  const uint32_t nn_queries = args.nn_queries, epw = args.epw, carry_fit_lo = args.carry_fit_lo;
  const float fit_fill = args.fit_fill;
  __shared__ unsigned int s_waves, s_edges, s_steered;
  if (step_cnt && threadIdx.x < 2u * (uint32_t(kMaxSteps) + 1u)) step_cnt[threadIdx.x] = 0u;
  // per-problem inputs of the batch rule, cached once (the fit evaluates it eleven times per problem) and the three count
  // arrays, scanned in LDS; problems beyond the cache capacity fall back to global memory
  constexpr uint32_t kCache = 1024;
  __shared__ float s_bf[kCache], s_sq[kCache];
  __shared__ uint32_t s_bmin[kCache], s_bcap[kCache], s_probe_waves[kCache], s_probes[kCache], s_carried[kCache];
  __shared__ uint32_t s_scan[3][2 * kCache + 1];
  const bool cached = P <= kCache;
  const uint32_t tid = threadIdx.x;
  // With the wave fit on, a problem's candidates are a whole number of 32-edge steer waves: every (problem, candidates)
  // segment of the steer grid otherwise ends in a wave that is half empty on average (256 such waves per round of ~2700).
  const uint32_t granule = fit_fill > 0.0f ? epw : 1u;
  if (cached) {
    for (uint32_t i = tid; i < P; i += blockDim.x) {
      const PlannerState* st = probs[i].st;
      const BatchInputs in = batch_inputs(st);
      s_bf[i] = in.batch_factor;
      s_sq[i] = in.sqrt_n;
      s_bmin[i] = in.b_min;
      s_bcap[i] = in.b_cap;
      s_probe_waves[i] = round_waves(st->n_new, epw);
      s_probes[i] = st->n_new;
      s_carried[i] = st->carried;
    }
    __syncthreads();
  }
  // A round that carries (round_carry.h) runs launch 0 over one compact list of the edges it steers: its waves are that
  // total over epw, rounded up, with the expected reuse taken off every problem's candidates.
  auto waves_at = [&](float sc) -> uint32_t {  // block-wide sum, same value in every thread
    uint32_t w = 0, e = 0, steered = 0;
    for (uint32_t i = tid; i < P; i += blockDim.x) {
      uint32_t B, n_new, carried;
      if (cached) {
        B = round_batch(BatchInputs{s_bf[i], s_sq[i], s_bmin[i], s_bcap[i]}, sc, granule);
        n_new = s_probes[i];
        carried = s_carried[i];
        w += round_waves(B, epw) + s_probe_waves[i];
      } else {
        const PlannerState* st = probs[i].st;
        B = round_batch(batch_inputs(st), sc, granule);
        n_new = st->n_new;
        carried = st->carried;
        w += round_waves(B, epw) + round_waves(n_new, epw);
      }
      e += B + n_new;
      steered += B - carry_expected_reuse(carried, B) + n_new;
    }
    __syncthreads();
    if (tid == 0) s_waves = s_edges = s_steered = 0u;
    __syncthreads();
    if (w) atomicAdd(&s_waves, w);
    if (carry_fit_lo != kCarryOff && e) {
      atomicAdd(&s_edges, e);
      atomicAdd(&s_steered, steered);
    }
    __syncthreads();
    if (carry_fit_lo != kCarryOff && s_edges >= carry_fit_lo) return round_waves(s_steered, epw);
    return s_waves;
  };
  const float scale = fit_fill > 0.0f ? fit_batch_scale(waves_at, slots, fit_fill) : 1.0f;
  if (tid == 0) sel[parity ^ 1u] = 0u;
  uint32_t edges = 0;
  for (uint32_t i = tid; i < P; i += blockDim.x) {
    const ProblemDev pr = probs[i];
    PlannerState* st = pr.st;
    if (pr.round_n) pr.round_n[round_slot] = st->done ? 0u : st->n;
    const uint32_t B = round_batch(batch_inputs(st), scale, granule);
    if (!st->done && B == 0) st->done = 2;  // sample stream exhausted: host must upload more
    st->B = B;
    st->F = B;
    if (pr.round_n) pr.round_n[kProfRounds + round_slot] = B;  // second half of the profile array: queries of the round
    if (B) {
      st->rounds += 1;
      st->edges_speculated += B;
    }
    edges += B + st->n_new;
    // counts of the three compact launch mappings (scanned below): steer waves (pair_kernel_edges_per_wave() edges each) per (candidates | probes) segment of
    // the two-lanes steer kernel, single edges per segment of the one-wave-per-edge kernel, query blocks of the NN sweep
    uint32_t* wb = cached ? s_scan[0] : wave_base;
    uint32_t* eb = cached ? s_scan[1] : edge_base;
    uint32_t* nb = cached ? s_scan[2] : nn_base;
    if (wave_base) {
      wb[2 * i + 1] = round_waves(B, epw);
      wb[2 * i + 2] = round_waves(st->n_new, epw);
    }
    if (nn_base) nb[i + 1] = round_waves(B, nn_queries);
    if (edge_base) {
      eb[2 * i + 1] = B;
      eb[2 * i + 2] = st->n_new;
    }
  }
  if (edges) atomicAdd(&sel[parity], edges);
  __syncthreads();
  // exclusive prefixes in place (entry 0 = 0, last entry = total), one wave each; in LDS when cached, then copied out
  {
    uint32_t* wb = cached ? s_scan[0] : wave_base;
    uint32_t* eb = cached ? s_scan[1] : edge_base;
    uint32_t* nb = cached ? s_scan[2] : nn_base;
    // by one whole wave: every lane sums a contiguous stretch of the counts a[1 .. n], the wave scans the 64 sums, and
    // the lane writes its stretch's running totals (unsigned sums: the values do not depend on the grouping)
    auto scan = [&](uint32_t* a, uint32_t n) {
      const uint32_t lane = tid & 63u;
      const uint32_t len = (n + 63u) / 64u;
      const uint32_t k0 = 1u + lane * len;
      const uint32_t k1 = k0 + len < n + 1u ? k0 + len : n + 1u;  // the stretch [k0, k1); empty beyond n
      uint32_t s = 0;
      for (uint32_t k = k0; k < k1; ++k) s += a[k];
      uint32_t incl = s;
#pragma unroll
      for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      uint32_t acc = incl - s;
      for (uint32_t k = k0; k < k1; ++k) {
        acc += a[k];
        a[k] = acc;
      }
      if (lane == 0) a[0] = 0;
    };
    const uint32_t wave = tid >> 6;  // (uniform per wave: all of its lanes scan)
    if (wave_base && wave == 0) scan(wb, 2 * P);
    if (edge_base && wave == 2) scan(eb, 2 * P);
    if (nn_base && wave == 1) scan(nb, P);
    if (cached) {
      __syncthreads();
      for (uint32_t k = tid; k <= 2 * P; k += blockDim.x) {
        if (wave_base) wave_base[k] = s_scan[0][k];
        if (edge_base) edge_base[k] = s_scan[1][k];
        if (nn_base && k <= P) nn_base[k] = s_scan[2][k];
      }
    }
  }
}

// One wave per candidate b: smallest squared distance from sample b to the end states of accepted
// candidates j < b.  min_j sqrt(s_j) == sqrt(min_j s_j) (sqrt is monotone), so one sqrt decides.
template <int DP>
__global__ __launch_bounds__(256) void fixup_kernel(const ProblemDev* __restrict__ probs, int D) {
  const ProblemDev pr = probs[blockIdx.y];
  PlannerState* st = pr.st;
  const uint32_t B = st->B;
  const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B || b == 0) return;
  const double* q = pr.samples + (uint64_t(st->s0) + b) * D;
  double qv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = d < D ? q[d] : 0.0;
  double smin = INFINITY;
  for (uint32_t j = lane; j < b; j += 64) {
    if (!pr.accept[j]) continue;
    const double* p = pr.x_out + uint64_t(j) * D;
    const double s = nn_exact_sq<DP>([&](int d) { return qv[d] - nn_qcoord(p, d, D); });
    if (s < smin) smin = s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(smin, off, 64);
    if (o < smin) smin = o;
  }
  if (lane == 0 && sqrt(smin) < pr.nn_dist[b]) atomicMin(&st->F, b);
}

// The same verdict with every accepted end state read from global memory once per block and row tile instead of once per
// candidate: a block takes kFixCands consecutive candidates of one problem, lane l of each of its four waves candidate
// b0 + l, and walks the rows below them in tiles of fix_rows<DP>().  Of a tile only the ACCEPTED rows are staged in LDS,
// packed in row order (ballot per wave, prefix over the waves), with their row numbers; wave w then takes the staged
// rows w, w + 4, ... -- all lanes read the same row, an LDS broadcast -- and a lane keeps a row's distance if the row
// lies below its candidate.  The four waves' minima meet in LDS.  A minimum does not depend on the order, every distance
// is nn_exact_sq of the same operands: F is what fixup_kernel finds.
constexpr uint32_t kFixCands = 64;
template <int DP>
constexpr uint32_t fix_rows() { return DP <= 16 ? 256u : 128u; }  // 24 .. 32 KB of rows per block

template <int DP>
__global__ __launch_bounds__(256) void fixup_tiled_kernel(const ProblemDev* __restrict__ probs, int D) {
  constexpr uint32_t TR = fix_rows<DP>();
  __shared__ __attribute__((aligned(16))) double s_row[TR][DP];
  __shared__ uint32_t s_j[TR];
  __shared__ uint32_t s_cnt[4];
  __shared__ double s_min[4][kFixCands];
  __shared__ uint32_t s_F;
  const ProblemDev pr = probs[blockIdx.y];
  PlannerState* st = pr.st;
  const uint32_t B = st->B;
  const uint32_t b0 = blockIdx.x * kFixCands;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (b0 >= B) return;  // (uniform: B and b0 are the block's)
  // F only ever decreases (atomicMin), down to the smallest candidate whose test succeeds.  If the value read here is
  // at or below b0, the final F is too, and no candidate of this tile can lower it: the tile is not needed.  A stale
  // (larger) value only means the tile is evaluated although it could have been skipped.  Other blocks of the problem
  // lower F while this one starts, so ONE thread reads it and the whole block decides on that word: the exit is
  // block-uniform, no wave meets a barrier the others have left.
  if (tid == 0) s_F = st->F;
  __syncthreads();
  if (b0 >= s_F) return;
  const uint32_t b = b0 + lane;  // (b >= B, b == 0: no row lies below, or the result is not used)
  const uint32_t b_end = b0 + kFixCands < B ? b0 + kFixCands : B;
  const uint32_t j_end = b_end - 1u;  // rows [0, j_end) lie below some candidate of the tile
  const double* q = pr.samples + (uint64_t(st->s0) + (b < B ? b : b0)) * D;
  double qv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = d < D ? q[d] : 0.0;
  double smin = INFINITY;
  for (uint32_t r0 = 0; r0 < j_end; r0 += TR) {
    const uint32_t j = r0 + tid;
    const bool acc = tid < TR && j < j_end && pr.accept[j] != 0;
    const unsigned long long m = __ballot(acc);
    if (lane == 0) s_cnt[wave] = uint32_t(__builtin_popcountll(m));
    __syncthreads();
    uint32_t slot = uint32_t(__builtin_popcountll(m & ((1ull << lane) - 1ull)));
    for (uint32_t w = 0; w < wave; ++w) slot += s_cnt[w];
    const uint32_t staged = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (acc) {
      const double* p = pr.x_out + uint64_t(j) * D;
#pragma unroll
      for (int d = 0; d < DP; ++d) s_row[slot][d] = nn_qcoord(p, d, D);
      s_j[slot] = j;
    }
    __syncthreads();
    for (uint32_t k = wave; k < staged; k += 4) {
      const double* __restrict__ x = s_row[k];
      const double s = nn_exact_sq<DP>([&](int d) { return qv[d] - x[d]; });
      if (s_j[k] < b && s < smin) smin = s;
    }
    __syncthreads();  // (the next tile overwrites the staged rows and counts)
  }
  s_min[wave][lane] = smin;
  __syncthreads();
  if (wave == 0) {
    smin = s_min[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double o = s_min[w][lane];
      if (o < smin) smin = o;
    }
    const bool hit = b < B && sqrt(smin) < pr.nn_dist[b < B ? b : 0u];
    // lanes are candidates in order: the first hit is the tile's smallest
    const unsigned long long hits = __ballot(hit);
    if (hits && lane == uint32_t(__builtin_ctzll(hits))) atomicMin(&st->F, b);
  }
}

// One 256-thread block per problem: commit candidates [0, F) in order (prefix scan of the accept flags),
// honouring the vertex budget of keep_going() (motion_planner_base.hpp:355-374).
// The goal probe of every vertex it commits is settled here where probe_certified (probe_reach.h) holds for the row being
// written -- goal_dist = +inf at once -- and the vertex otherwise joins the problem's list of open probes, in vertex order
// (round_plan.h, the granule rule: the entries the round's launch ran leave the list, what it left behind moves to the
// front).  probe_granule: 32 = one steer wave of the two-lanes mapping when the wave fit is on, else 1.
// stash: the candidates this round throws away, [cut, B), leave their results for the next round (round_carry.h).
__global__ __launch_bounds__(256) void commit_kernel(const ProblemDev* __restrict__ probs, int D, int DP,
                                                      uint32_t probe_granule, bool stash, const ProbeReachDev reach) {
  __shared__ uint32_t scan[256];
  __shared__ uint32_t carry, open_carry;
  __shared__ uint32_t cut;  // number of candidates actually consumed
  __shared__ uint32_t opened;  // committed vertices appended to the list
  const ProblemDev pr = probs[blockIdx.x];
  PlannerState* st = pr.st;
  const uint32_t F = st->F;
  const uint32_t n0 = st->n;
  const uint32_t s0 = st->s0;
  const uint32_t budget = st->max_total - n0;  // vertices that may still be added
  const uint32_t B = st->B;
  const bool was_done = st->done != 0u;  // (read by every thread before thread 0 may change it below)
  // the round's launch ran the first n_new entries of the list; the `waited` ones behind them move to the front
  const uint32_t ran = st->n_new;
  const uint32_t waited = st->list_n - ran;
  const double reach_q = *reach.round_edges >= reach.min_edges ? reach.reach_q : INFINITY;
  if (threadIdx.x == 0) {
    carry = open_carry = 0;
    cut = F;
    opened = 0;
  }
  for (uint32_t base = 0; base < waited; base += 256) {  // (uniform; dest < src: read, barrier, write)
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < waited ? pr.probe_list[ran + k] : 0u;
    __syncthreads();
    if (k < waited) pr.probe_list[k] = v;
  }
  __syncthreads();
  for (uint32_t base = 0; base < F; base += 256) {
    const uint32_t b = base + threadIdx.x;
    const uint32_t a = (b < F && pr.accept[b]) ? 1u : 0u;
    // an accepted candidate whose goal probe stays open; both counts are scanned in one word (at most 256 each per pass)
    const uint32_t o =
        (a && !probe_certified(pr.x_out + uint64_t(b) * D, pr.goal, D, reach_q, reach.v_lower, reach.v_upper)) ? 1u : 0u;
    scan[threadIdx.x] = a | (o << 16);
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {  // Hillis-Steele inclusive scan
      uint32_t v = 0;
      if (threadIdx.x >= off) v = scan[threadIdx.x - off];
      __syncthreads();
      scan[threadIdx.x] += v;
      __syncthreads();
    }
    const uint32_t incl = carry + (scan[threadIdx.x] & 0xFFFFu);       // accepted among [0, b]
    const uint32_t open_incl = open_carry + (scan[threadIdx.x] >> 16);  // ... of them, with an open probe
    if (b < F) {
      // the candidate whose vertex exhausts the budget is the last one the sequential loop runs
      if (a && incl == budget) atomicMin(&cut, b + 1);
      if (incl <= budget && (incl < budget || a)) {
        // consumed by the sequential loop (it stops right after the budget-filling vertex)
        pr.nn_seq[s0 + b] = pr.nn_idx[b];
        pr.accept_log[s0 + b] = uint8_t(a);
        if (a) {
          const uint32_t row = n0 + incl - 1;
          for (int d = 0; d < DP; ++d) pr.tree[uint64_t(row) * DP + d] = d < D ? pr.x_out[uint64_t(b) * D + d] : 0.0;
          if (pr.mirror) mirror_store_row(pr.mirror, row, pr.x_out + uint64_t(b) * D, D, pr.mirror_scale, pr.dx_max_bits);
          pr.parent[row] = pr.nn_idx[b];
          pr.node_sample[row] = s0 + b;
          if (o) {
            pr.probe_list[waited + open_incl - 1] = row;
            atomicMax(&opened, open_incl);
          } else {
            pr.goal_dist[row - 1] = INFINITY;  // what goal_probe_steerable would leave
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 255) {
      carry = incl;
      open_carry = open_incl;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t added = carry < budget ? carry : budget;
    const uint32_t n = n0 + added;
    st->n = n;
    const uint32_t list_n = waited + opened;
    st->list_n = list_n;
    st->n_new = probe_ride_count(list_n, waited, probe_granule);
    st->probed_n = probe_probed_n(pr.probe_list, list_n, n);
    st->probes_run += ran;
    st->probes_certified += added - opened;
    st->s0 = s0 + cut;
    st->fixup_cut += (B - F);
    st->cand_discarded += (B - cut);
    if (st->n >= st->max_total) st->done = 1;
  }
  // rows [cut, B) of the round's results -> the stash, packed from slot 0.  Every candidate of the round was steered (or
  // took a stashed result itself), whichever mapping ran, so every row is the result of (nn_idx[b], sample s0 + b).
  const uint32_t added_all = carry < budget ? carry : budget;
  const bool live = !was_done && n0 + added_all < st->max_total;
  const uint32_t carried = carry_count(B, cut, stash && pr.stash_x && live);
  if (threadIdx.x == 0) st->carried = carried;
  for (uint32_t j = threadIdx.x; j < carried; j += 256) {
    const uint32_t b = carry_old_slot(j, cut);
    pr.stash_nn[j] = pr.nn_idx[b];
    pr.stash_steps[j] = pr.steps[b];
    pr.stash_accept[j] = pr.accept[b];
  }
  const double* __restrict__ x_from = pr.x_out + uint64_t(carry_old_slot(0u, cut)) * D;
  for (uint32_t k = threadIdx.x; k < carried * uint32_t(D); k += 256) pr.stash_x[k] = x_from[k];
}

// One block per problem, between the NN resolve and the steer launches of a round that carries (carry_round of the round's
// edge count: the same decision launch 0 of propagate_pair_step_kernel takes).  Candidates the reuse predicate marks take
// their stashed end state, accept bit and step count; every other candidate and every goal probe of the problem is
// appended to the list launch 0 reads, as (segment, edge, no carried clearance, 0): one ballot, one prefix and one atomic
// per wave.  A reused edge is in no list: no steer launch sees it.
__global__ __launch_bounds__(256) void carry_restore_kernel(const ProblemDev* __restrict__ probs, int D,
                                                             const uint32_t* __restrict__ edge_count, uint32_t lo, uint32_t hi,
                                                             uint32_t carry_min_edges, uint4* __restrict__ list,
                                                             uint32_t* __restrict__ list_cnt, uint32_t list_cap) {
  if (!carry_round(*edge_count, lo, hi, carry_min_edges)) return;
  const ProblemDev pr = probs[blockIdx.x];
  PlannerState* st = pr.st;
  const uint32_t B = st->B, n_new = st->n_new, carried = st->carried;
  const uint32_t total = B + n_new;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t n_reused = 0;  // (lane 0 of each wave counts its wave's)
  for (uint32_t base = 0; base < total; base += 256) {  // (uniform trip count)
    const uint32_t i = base + threadIdx.x;
    const bool cand = i < B;
    const bool reuse = cand && carry_reuses(i, carried, B, pr.nn_idx[i], pr.stash_nn);
    if (reuse) {
      for (int d = 0; d < D; ++d) pr.x_out[uint64_t(i) * D + d] = pr.stash_x[uint64_t(i) * D + d];
      pr.accept[i] = pr.stash_accept[i];
      pr.steps[i] = pr.stash_steps[i];
    }
    const bool steered = i < total && !reuse;
    const unsigned long long m = __ballot(steered);
    n_reused += uint32_t(__popcll(__ballot(reuse)));
    if (m) {
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(list_cnt, uint32_t(__popcll(m)));
      at = uint32_t(__builtin_amdgcn_readfirstlane(int(at))) + uint32_t(__popcll(m & below));
      if (steered && at < list_cap) list[at] = make_uint4(2u * blockIdx.x + (cand ? 0u : 1u), cand ? i : i - B, 0u, 0u);
    }
  }
  if (lane == 0 && n_reused) atomicAdd(&st->cand_reused, (unsigned long long)n_reused);
}

// The sample stream is generated ON THE DEVICE: hyperbox_topology::random_point (hyperbox_topology.hpp:97-103) draws D
// times uniform_01<mt19937&, double> = eng() * 2^-32 per sample (Boost.Random on a 32-bit engine: one draw per
// coordinate), so draw number k * D + d is coordinate d of sample k whatever happens in the planner.  One block per
// problem keeps that problem's mt19937 state (624 words + position, global_rng.hpp:44-54 seeded like std::mt19937) in LDS,
// regenerates it 624 words at a time in the three data-parallel stretches of the recurrence (words 0..226 read only old
// words, 227..453 the new 0..226, 454..622 the new 227..395, word 623 the new 396 and 0) and writes the samples behind the
// ones the rounds may read; only then it raises the problem's samples_ready (a round that still sees the old value just
// takes a smaller batch).  (Round 1 generated the stream on one host thread and uploaded it: ~15 M draws per 16 rounds,
// as long as the GPU needed for those rounds.)
struct SampleSeg {
  double* dst;           // first new sample of the problem
  uint64_t count;        // doubles to produce (a multiple of D)
  uint32_t* mt;          // the problem's generator: 624 state words + position
  uint32_t* ready_ptr;   // &PlannerState::samples_ready of the problem
  uint32_t ready_new;
  uint32_t pad;
};
constexpr int kMtN = 624, kMtM = 397;
__device__ __forceinline__ uint32_t mt_twist(uint32_t cur, uint32_t nxt, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (nxt & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__global__ __launch_bounds__(256) void generate_samples_kernel(const SampleSeg* __restrict__ tab,
                                                                const double* __restrict__ bounds, int D) {
  __shared__ uint32_t mt[kMtN];
  const SampleSeg sg = tab[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < uint32_t(kMtN); i += 256) mt[i] = sg.mt[i];
  uint32_t idx = sg.mt[kMtN];
  __syncthreads();
  uint64_t produced = 0;
  while (produced < sg.count) {  // uniform
    if (idx == uint32_t(kMtN)) {
      // words [a, b): new[i] = twist(old[i], old[i + 1], word (i + 397) mod 624 as it stands at this point)
      auto stretch = [&](uint32_t a, uint32_t b) {
        const uint32_t i = a + tid;
        uint32_t v = 0;
        if (i < b) v = mt_twist(mt[i], mt[i + 1], mt[i + kMtM < uint32_t(kMtN) ? i + kMtM : i + kMtM - kMtN]);
        __syncthreads();  // every thread has read its old neighbour before anybody overwrites it
        if (i < b) mt[i] = v;
        __syncthreads();
      };
      stretch(0, kMtN - kMtM);                  // 0 .. 226
      stretch(kMtN - kMtM, 2 * (kMtN - kMtM));  // 227 .. 453
      stretch(2 * (kMtN - kMtM), kMtN - 1);     // 454 .. 622
      if (tid == 0) mt[kMtN - 1] = mt_twist(mt[kMtN - 1], mt[0], mt[kMtM - 1]);
      __syncthreads();
      idx = 0;
    }
    const uint64_t left = sg.count - produced;
    const uint32_t chunk = (uint64_t(kMtN - idx) < left) ? uint32_t(kMtN - idx) : uint32_t(left);
    for (uint32_t t = tid; t < chunk; t += 256) {
      uint32_t y = mt[idx + t];
      y ^= (y >> 11);
      y ^= (y << 7) & 0x9d2c5680u;
      y ^= (y << 15) & 0xefc60000u;
      y ^= (y >> 18);
      const double u = double(y) * (1.0 / 4294967296.0);  // < 1 for every 32-bit y: uniform_01 never redraws
      const int d = int((produced + t) % uint64_t(D));
      sg.dst[produced + t] = bounds[d] + u * (bounds[D + d] - bounds[d]);
    }
    produced += chunk;
    idx += chunk;
    __syncthreads();
  }
  for (uint32_t i = tid; i < uint32_t(kMtN); i += 256) sg.mt[i] = mt[i];
  if (tid == 0) sg.mt[kMtN] = idx;
  __threadfence();  // the samples are visible device-wide before the count says so
  __syncthreads();
  if (tid == 0) *sg.ready_ptr = sg.ready_new;
}

// Goal-probe results since the last sync: block b copies problem b's new stretch into one buffer (one device->host copy
// for all problems instead of one per problem).
struct GoalSeg {
  const double* src;
  uint64_t dst_off, count;
};
__global__ __launch_bounds__(256) void gather_goal_dist_kernel(const GoalSeg* __restrict__ tab, double* __restrict__ out) {
  const GoalSeg g = tab[blockIdx.x];
  for (uint64_t i = threadIdx.x; i < g.count; i += 256) out[g.dst_off + i] = g.src[i];
}

// before the flush launch: every pending probe rides, whatever the granule
__global__ void probes_take_all_kernel(const ProblemDev* __restrict__ probs) {
  if (threadIdx.x != 0) return;
  PlannerState* st = probs[blockIdx.x].st;
  st->n_new = st->list_n;
}

// after a probe-only flush launch: the list is empty, every vertex has its result
__global__ void probes_flushed_kernel(const ProblemDev* __restrict__ probs) {
  if (threadIdx.x != 0) return;
  PlannerState* st = probs[blockIdx.x].st;
  st->probes_run += st->n_new;
  st->probed_n = st->n;
  st->list_n = 0;
  st->n_new = 0;
}


// ---- create: one init pass over all problems ---------------------------------------------------------------------------
// The planner's memory is a range of an arena that may have served another planner before: whatever a kernel reads before
// a kernel writes it is written here.
struct ProblemInit {  // one problem's row of the init table
  uint32_t* mt;           // its generator: 624 state words + position
  double* tree;           // row 0 = the start state, padded with zeroes to DP
  uint32_t* parent;       // parent[0] = none
  double* goal;
  uint32_t* seed_row;     // [b_max] NnArgs::seed: all ones between sweeps
  uint32_t* cand;         // scratch of the mirror sweep + the mirror's error word: zero (null without a mirror)
  uint4* mirror;          // pad rows everywhere, then the root's row
  uint32_t* dx_max_bits;
  uint64_t mirror_frags;  // 16-byte fragments of the mirror
  double mirror_scale;    // the prescale its rows are written with
  uint32_t seed, pad;
  double start[RKH_MAX_STATE], goal_x[RKH_MAX_STATE];
};

// blockIdx.y = problem; the blocks of a problem stride over its mirror
__global__ __launch_bounds__(256) void mirror_fill_all_kernel(const ProblemInit* __restrict__ tab) {
  uint4* const mirror = tab[blockIdx.y].mirror;
  const uint64_t frags = tab[blockIdx.y].mirror_frags;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < frags; i += gridDim.x * 256ull) mirror[i] = mirror_pad_fragment(i);
}

// One block per problem, after mirror_fill_all_kernel.  get_global_rng().seed(s): std::mt19937 / boost::mt19937 seeding
// (32-bit integer recurrence), position at the end of the state.
__global__ __launch_bounds__(256) void planner_init_kernel(const ProblemInit* __restrict__ tab, int D, int DP, uint32_t b_max,
                                                            uint32_t cand_words) {
  const ProblemInit& pi = tab[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = tid; k < b_max; k += 256) pi.seed_row[k] = 0xFFFFFFFFu;
  for (uint32_t k = tid; k < cand_words; k += 256) pi.cand[k] = 0u;
  if (tid < uint32_t(DP)) pi.tree[tid] = tid < uint32_t(D) ? pi.start[tid] : 0.0;
  if (tid < uint32_t(D)) pi.goal[tid] = pi.goal_x[tid];
  if (tid == 64) pi.parent[0] = 0xFFFFFFFFu;
  if (tid == 128) {
    uint32_t w = pi.seed;
    pi.mt[0] = w;
    for (uint32_t k = 1; k < uint32_t(kMtN); ++k) {
      w = 1812433253u * (w ^ (w >> 30)) + k;
      pi.mt[k] = w;
    }
    pi.mt[kMtN] = uint32_t(kMtN);
  }
  __syncthreads();  // the error word is zero before the root's row raises it
  if (tid == 0 && pi.mirror) mirror_store_row(pi.mirror, 0, pi.start, D, pi.mirror_scale, pi.dx_max_bits);
}

}  // namespace rkh

using namespace rkh;

namespace {
struct Problem {  // host view of one planning problem
  rkh_rrt_params prm;
  // ranges of the planner's arena (planner_arena_layout, ProblemRange), set by alloc_planner_buffers
  uint32_t* d_mt = nullptr;  // the problem's mt19937 on the device: 624 state words + position
  double *d_tree = nullptr, *d_goal_dist = nullptr, *d_goal = nullptr;  // [capacity] vertex rows and goal-probe results; the goal
  uint32_t *d_parent = nullptr, *d_node_sample = nullptr;               // [capacity]
  double* d_samples = nullptr;                                          // [sample_cap] the sample stream ...
  uint32_t* d_nn_seq = nullptr;                                         // ... and the log of its iterations
  uint8_t* d_accept_log = nullptr;
  uint32_t *d_nn_idx = nullptr, *d_steps = nullptr, *d_probe_steps = nullptr;  // [b_max (+ kProbeGranule)] a round's candidates and probes
  double *d_nn_dist = nullptr, *d_x_out = nullptr, *d_probe_x = nullptr;
  uint8_t* d_accept = nullptr;
  uint32_t* d_probe_list = nullptr;  // [b_max + kProbeGranule] vertices whose goal probe is open, in vertex order
  double* d_stash_x = nullptr;  // [b_max] the last round's discarded candidates (round_carry.h); null: no carry
  uint32_t *d_stash_nn = nullptr, *d_stash_steps = nullptr;
  uint8_t* d_stash_accept = nullptr;
  double* d_part_dist = nullptr;                                        // partial minima of the NN sweep
  uint32_t *d_part_idx = nullptr, *d_round_n = nullptr;
  void* d_mirror = nullptr;          // half-precision mirror of d_tree (nn_mirror.h)
  void* d_cand = nullptr;            // per-query scratch of the mirror sweep (nn1_mirror_carve), then one word:
  uint32_t* dx_max_bits = nullptr;   // ... this one, the mirror's running maximum of |x - x_h| (null without a mirror)
  // the three stream buffers once they have grown (grow_sample_buffers): d_samples, d_nn_seq and d_accept_log then point
  // into these and the arena's ranges lie idle
  DeviceBuffer<double> grown_samples;
  DeviceBuffer<uint32_t> grown_nn_seq;
  DeviceBuffer<uint8_t> grown_accept_log;
  uint64_t capacity = 0, sample_cap = 0, samples_ready = 0;
  PlannerState h_state;
  // solution bookkeeping (register_basic_solution_path_impl, solution_path_factories.hpp:58-110)
  uint64_t goal_checked = 0;
  uint64_t num_solutions = 0;
  double best_cost = INFINITY;
  uint32_t best_vertex = 0xFFFFFFFFu;  // vertex whose goal probe gave the best registered solution
  bool truncated = false;
  uint64_t final_n = 0, final_iterations = 0;
};
static_assert(std::is_nothrow_move_constructible<Problem>::value, "std::vector<Problem> is resized");
}  // namespace

struct rkh_planner {
  rkh_scene* scene = nullptr;
  hipStream_t stream = nullptr;
  // All device memory of the handle but the grown stream buffers and d_gd: one slab, carved by planner_arena_layout.  It
  // comes from the scene's context and goes back to it (arena_cache: RKH_ARENA_CACHE=0 at create turns that off).
  DeviceArena arena;
  rkh_ctx* ctx = nullptr;  // the scene's, as it was at create: the arena goes back to it if it still exists
  ArenaLayout layout;
  bool arena_cache = true;    // RKH_ARENA_CACHE
  bool arena_poison = false;  // RKH_ARENA_POISON: the slab is filled with 0xA5 bytes before anything is written
  // One pinned block: the image of the arena's upload ranges [0, layout.upload_bytes) that create copies to the device
  // (rkh_planner_sync then reads the states back into their place in it), the error flag's read-back slot, the two segment
  // tables of the sample generator and the one of the goal-probe gather.
  PinnedBuffer<char> h_block;
  int* h_err = nullptr;
  PinnedBuffer<double> h_gd;  // pinned read-back buffer of the goal-probe results (rkh_planner_sync)
  hipStream_t copy_stream = nullptr;  // sample-stream uploads (beside the rounds enqueued on `stream`)
  bool quasi_static = false;  // false: steerable dynamic space (propagate kernel); true: manip_quasi_static_env (edge_check)
  double lower[RKH_MAX_STATE], upper[RKH_MAX_STATE];  // hyperbox the samples are drawn from
  DynDev dyn;
  QsDev qs;
  int n_dof = 0, D = 0, DP = 0;
  uint32_t P = 0;
  std::vector<Problem> prob;
  uint32_t b_max = 1024;
  uint32_t b_min = 8;          // RKH_BATCH_MIN
  float batch_factor = 1.25f;  // candidates per round = batch_factor * sqrt(n) per problem (tune_planner)
  uint64_t sample_cap_min = 0;  // RKH_SAMPLE_CAP: at least this many samples in a problem's first stream buffers
  SteerMapping steer = SteerMapping::Wave;  // the form of every round's steer launches (steer_mapping; dynamic space)
  double* d_lane_ws = nullptr;  // workspace of the two-lanes-per-edge kernel
  double coord_bound = 0.0;     // max |coordinate| of vertices and samples (hyperbox bounds), 0 = unknown
  uint32_t* d_sel = nullptr;        // [2] edges of the current round (by round parity), see round_begin_kernel
  uint32_t* d_nn_base = nullptr;    // [P + 1] prefix of the NN sweep's query blocks per problem (matrix-core kernel)
  uint32_t* d_wave_base = nullptr;  // [2 P + 1] prefix of the working waves per (problem, candidates | probes) segment
  uint32_t* d_edge_base = nullptr;  // [2 P + 1] ... of the single edges per segment (behind d_wave_base in its range)
  uint32_t round_parity = 0;
  // host-side upper bounds that size the launches of a round (the exact counts live on the device): n_ub[i] >= vertex
  // count of problem i (exact after every sync, + the round's batch bound per enqueued round)
  std::vector<uint64_t> n_ub;
  uint32_t prev_batch_ub = 0;  // batch bound of the previous round = bound on this round's goal probes
  int wave_fit = 1;          // per-round batch scale chosen on the device (round_begin_kernel); RKH_WAVE_FIT=0: off
  double wave_fill = 0.99;   // target fill of the last pass of steer waves (RKH_WAVE_FILL)
  uint32_t wave_slots = 1024;    // SIMDs of the device = concurrent waves of the two-lanes steer kernel
  uint32_t duo_threshold = 0;     // Auto rounds below this many edges: two waves per edge (RKH_DUO_THRESHOLD; 0 = never)
  uint32_t lane_threshold = 1024;  // rounds with at least this many edges go to the two-lanes-per-edge kernel (one wave-per-edge pass fills the 1024 SIMDs; measured optimum at 4, 16 and 32 problems, tests/diag_lane_threshold.sh)
  uint32_t part_blocks = 0;
  uint64_t max_capacity = 0;
  // device tables (P entries each)
  PlannerState* d_states = nullptr;
  ProblemDev* d_probs = nullptr;
  NnArgs* d_nn_args = nullptr;
  EdgeIO* d_io_steer = nullptr;
  EdgeIO* d_io_probe = nullptr;
  bool nn_mirror = false;  // the NN search of a round runs over the trees' half-precision mirrors (nn_mirror.hip)
  double mirror_scale = 1.0;  // ... written in units of this power of two (mirror_prescale(coord_bound))
  bool nn_open = true;     // ... its second pass only where a query is open (RKH_NN_MIRROR_OPEN)
  bool fixup_tiled = true; // the fix-up stages accepted end states in LDS (RKH_FIXUP_TILED; 0: one wave per candidate)
  double x_norm_bound = 0.0;  // >= |x| of every vertex (hyperbox corners, start states)
  // Step-wise steer launches (propagate_pair_step_kernel): one launch per RK4 step over the live edges of all problems,
  // survivors handed on through two ping-pong lists.
  uint4* d_step_list[2] = {nullptr, nullptr};  // (segment, edge, carried clearance) of the edges alive after step k (k odd / even)
  uint32_t step_list_cap = 0;          // entries of each list
  uint32_t* d_step_cnt = nullptr;      // [2 (kMaxSteps + 1)] front, then back entries of the list launch k reads (cleared by round_begin_kernel)
  bool steer_clearance = true;         // RKH_STEER_CLEARANCE
  unsigned long long* d_steps_exec = nullptr;  // edge-steps integrated by the steer kernels (diagnostics: rkh_planner_steer_steps)
  uint32_t step_blocks_cap = 0;                // grid bound of a step launch (its blocks stride over the chunks beyond it)
  // rounds below this many edges keep the single whole-edge launch of the two-lanes mapping (RKH_STEER_SPLIT_MIN_EDGES;
  // default: what leaves every SIMD at most one 32-edge wave -- such a round gains nothing from shedding waves)
  uint32_t split_min_edges = 0;
  // Rounds that take the step-wise launch with at least carry_min_edges edges reuse the steered edges of the candidates
  // the round before discarded (round_carry.h; RKH_STEER_CARRY=0: never, RKH_STEER_CARRY_MIN_EDGES).  The default is the
  // built-in step-wise threshold whatever split_min_edges says: only the step-wise launches honour the mark, and the
  // executed-step counter stays comparable across the mappings below it.
  bool carry = false;
  uint32_t carry_min_edges = 0;
  // the wave fit takes the expected reuse off a carrying round's work: measured 0.5 % slower than counting the candidates
  // (DESIGN 5), so off unless RKH_STEER_CARRY_FIT=1 asks for it
  bool carry_fit = false;
  // Goal probes that cannot reach the goal are settled at commit (probe_reach.h): the travel bound of this scene and
  // space, computed once at create.  reach_q = +inf -- the quasi-static space, every scene outside probe_travel's
  // conditions, RKH_PROBE_REACH=0 -- certifies nothing: every vertex's probe is steered.
  ProbeReachDev reach;
  uint64_t max_n_ub = 1;  // largest vertex-count bound over the problems (sizes the mirror sweep's row slices)
  uint64_t sum_batch_ub = 0, prev_sum_batch_ub = 0;  // host-side bounds on the candidates of this / the previous round, all problems
  // segment tables of the sample generator: [0] what the enqueued rounds need, [1] the next call's share, generated
  // while the GPU works on the rounds just enqueued
  double* d_bounds = nullptr;  // lower[D], upper[D] of the sampled hyperbox
  struct Staging {
    SampleSeg* h_tab = nullptr;  // pinned segment table [P] (h_block)
    SampleSeg* d_tab = nullptr;
    hipEvent_t done = nullptr;
    bool pending = false;
  } staging[2];
  GoalSeg* h_gd_tab = nullptr;  // pinned [P] (h_block)
  GoalSeg* d_gd_tab = nullptr;
  DeviceBuffer<double> d_gd;       // gathered goal-probe results (rkh_planner_sync)
  // optional HIP-event timing of the NN sweep kernel (RKH_PROFILE_NN=1)
  bool profile_nn = false;
  std::vector<hipEvent_t> ev;  // pairs
  std::vector<hipEvent_t> ev_steer;  // pairs around the steer launches of the same rounds
  uint32_t prof_rounds = 0;
  static constexpr uint32_t kProfMax = kProfRounds;

  // the two-lanes steer kernel runs in this planner's rounds: its residency sizes the wave fit and the step-wise launches
  bool lane_kernel() const { return steer == SteerMapping::Auto || steer == SteerMapping::Pair; }

  // Both streams idle and the events gone first; the arena then goes back to the context and the members free the rest.
  ~rkh_planner() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (Staging& sg : staging) {
      if (sg.pending) (void)hipEventSynchronize(sg.done);
      if (sg.done) (void)hipEventDestroy(sg.done);
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_steer) (void)hipEventDestroy(e);
    if (copy_stream) {
      (void)hipStreamSynchronize(copy_stream);
      (void)hipStreamDestroy(copy_stream);
    }
    if (stream) (void)hipStreamDestroy(stream);
    if (arena_cache && ctx) ctx_give_arena(ctx, std::move(arena));
  }
};

namespace {

// Extend every problem's device-resident sample stream by `ahead` samples beyond its (last known) cursor
// (generate_samples_kernel).  The launch goes to the planner's second stream, beside the rounds already enqueued on the
// first one; the table's previous use is awaited through its event, so no stream synchronisation happens here.
rkh_status upload_samples_all(rkh_planner* p, uint64_t ahead, int which) {
  rkh_planner::Staging& sg = p->staging[which];
  const int D = p->D;
  std::vector<uint64_t> upto(p->P, 0);
  bool any = false;
  for (uint32_t i = 0; i < p->P; ++i) {
    Problem& q = p->prob[i];
    if (q.truncated || q.h_state.done == 1) continue;
    uint64_t want = uint64_t(q.h_state.s0) + ahead;
    if (want > q.sample_cap) want = q.sample_cap;
    if (want <= q.samples_ready) continue;
    upto[i] = want;
    any = true;
  }
  if (!any) return RKH_OK;
  if (sg.pending) {
    RKH_HIP(hipEventSynchronize(sg.done));
    sg.pending = false;
  }
  if (!sg.done) RKH_HIP(hipEventCreateWithFlags(&sg.done, hipEventDisableTiming));
  uint32_t n_seg = 0;
  for (uint32_t i = 0; i < p->P; ++i) {
    if (!upto[i]) continue;
    Problem& q = p->prob[i];
    SampleSeg& seg = sg.h_tab[n_seg++];
    seg.dst = q.d_samples + q.samples_ready * D;
    seg.count = (upto[i] - q.samples_ready) * D;
    seg.mt = q.d_mt;
    seg.ready_ptr = &p->d_states[i].samples_ready;
    seg.ready_new = uint32_t(upto[i]);
    seg.pad = 0;
    q.samples_ready = upto[i];
  }
  RKH_HIP(hipMemcpyAsync(sg.d_tab, sg.h_tab, n_seg * sizeof(SampleSeg), hipMemcpyHostToDevice, p->copy_stream));
  hipLaunchKernelGGL(generate_samples_kernel, dim3(n_seg), dim3(256), 0, p->copy_stream, sg.d_tab, p->d_bounds, D);
  RKH_HIP(hipGetLastError());
  // The generator runs on its own stream, beside the rounds already enqueued on the planner stream: it writes beyond every
  // problem's samples_ready (no round reads there) and then raises samples_ready.  Work enqueued on the planner stream
  // from here on waits for it.
  RKH_HIP(hipEventRecord(sg.done, p->copy_stream));
  RKH_HIP(hipStreamWaitEvent(p->stream, sg.done, 0));
  sg.pending = true;
  return RKH_OK;
}

// fix-up of a round's candidates against the vertices the round itself would add
rkh_status launch_fixup(rkh_planner* p, uint32_t batch_ub) {
  const bool dims_ok = with_padded_dims(p->DP, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if (p->fixup_tiled)
      hipLaunchKernelGGL((fixup_tiled_kernel<DP>), dim3((batch_ub + kFixCands - 1) / kFixCands, p->P), dim3(256), 0,
                         p->stream, p->d_probs, p->D);
    else
      hipLaunchKernelGGL((fixup_kernel<DP>), dim3((batch_ub + 3) / 4, p->P), dim3(256), 0, p->stream, p->d_probs, p->D);
  });
  if (!dims_ok) {
    set_error("planner: unsupported state dimension");
    return RKH_ERR_UNSUPPORTED;
  }
  return RKH_OK;
}

// upper bound of the batch round_begin_kernel will choose for a problem with at most n_ub vertices: the batch rule at the
// host's bounds, whatever the problem has left of its sample stream
uint32_t batch_upper_bound(const PlannerState& st, uint64_t n_ub, float batch_scale) {
  return round_batch(BatchInputs{st.batch_factor, sqrtf(float(n_ub)), st.b_min, st.b_max}, batch_scale, 1u);
}

// The steer plan of a launch of grid_a + grid_b edges per problem; compact: a regular round, over the (candidates, probes)
// segments round_begin_kernel counted.
SteerPlan auto_steer_plan(const rkh_planner* p, uint32_t grid_a, uint32_t grid_b, bool compact) {
  SteerPlanInputs in;
  in.lane_threshold = p->lane_threshold;
  in.duo_threshold = p->duo_threshold;
  in.split_min_edges = p->split_min_edges;
  in.carry_min_edges = p->carry ? p->carry_min_edges : kCarryOff;
  in.compact = compact && p->d_wave_base;
  in.stepwise = p->d_step_cnt && p->dyn.n_steps > 1;
  in.prismatic = p->scene->host.has_prismatic != 0;
  // candidates + pending probes of all problems
  in.edges_ub = std::min<uint64_t>(p->sum_batch_ub + p->prev_sum_batch_ub + uint64_t(p->P) * kProbeGranule,
                                   uint64_t(grid_a + grid_b) * p->P);
  return steer_plan(in);
}

// steer / probe edges of all problems: RK4 propagation (dynamic space) or the min_interval walk (quasi-static space).
// plan: auto_steer_plan of the same grid (only Auto planners look at it).
rkh_status launch_edges(rkh_planner* p, uint32_t grid_a, uint32_t grid_b, const EdgeIO* tab_a, const EdgeIO* tab_b,
                        const SteerPlan& plan) {
  if (p->quasi_static)
    return launch_edge_check(p->stream, *p->scene, p->qs, EdgeIO(), grid_a, grid_b, tab_a, tab_b, p->P);
  if (p->steer != SteerMapping::Auto) {
    KernelGate always;  // no gate; the executed steps are counted like Auto's (rkh_planner_steer_steps)
    always.steps_exec = p->d_steps_exec;
    always.clearance = p->steer_clearance;
    always.clear_stats = p->scene->d_clear_stats.get();
    return launch_propagate(p->stream, *p->scene, p->steer, p->dyn, EdgeIO(), grid_a, grid_b, tab_a, tab_b, p->P,
                            p->d_lane_ws, always);
  }
  for (uint32_t k = 0; k < plan.n; ++k) {
    const SteerLaunch& L = plan.launch[k];
    const bool lanes = L.form == SteerForm::LanesWhole || L.form == SteerForm::LanesSteps;
    KernelGate gate{p->d_sel + p->round_parity, L.lo, L.hi};
    gate.steps_exec = p->d_steps_exec;
    if (lanes) {
      gate.clearance = p->steer_clearance;
      gate.clear_stats = p->scene->d_clear_stats.get();
    }
    if (plan.in.compact) {  // the prefixes of round_begin_kernel: steer waves for the two-lanes forms, else single edges
      gate.wave_base = lanes ? p->d_wave_base : p->d_edge_base;
      gate.n_segments = 2 * p->P;
    }
    if (L.form != SteerForm::LanesSteps) {
      SteerMapping m = SteerMapping::Pair;
      if (L.form == SteerForm::TwoWaves) m = SteerMapping::Duo;
      if (L.form == SteerForm::OneWave) m = plan.in.prismatic ? SteerMapping::Prismatic : SteerMapping::Wave;
      RKH_TRY(launch_propagate(p->stream, *p->scene, m, p->dyn, EdgeIO(), grid_a, grid_b, tab_a, tab_b, p->P,
                               lanes ? p->d_lane_ws : nullptr, gate));
      continue;
    }
    const uint32_t epw = pair_kernel_edges_per_wave();
    const uint32_t blocks = uint32_t(std::min<uint64_t>((plan.in.edges_ub + epw - 1) / epw, p->step_blocks_cap));
    // a round that carries: the stashed results go to their slots and launch 0 gets the list of the edges left to steer
    if (plan.restore) {
      hipLaunchKernelGGL(carry_restore_kernel, dim3(p->P), dim3(256), 0, p->stream, p->d_probs, p->D, gate.count, gate.lo,
                         gate.hi, plan.in.carry_min_edges, p->d_step_list[0], p->d_step_cnt, p->step_list_cap);
    }
    RKH_TRY(launch_propagate_pair_steps(p->stream, *p->scene, p->dyn, tab_a, tab_b, p->P, p->d_edge_base,
                                        p->d_step_list[0], p->d_step_list[1], p->step_list_cap, p->d_step_cnt,
                                        p->d_lane_ws, blocks, gate, p->d_steps_exec, plan.in.carry_min_edges));
  }
  return RKH_OK;
}

// goal probes still pending after the last enqueued round
rkh_status flush_probes(rkh_planner* p) {
  hipLaunchKernelGGL(probes_take_all_kernel, dim3(p->P), dim3(64), 0, p->stream, p->d_probs);
  const uint32_t grid = p->b_max + kProbeGranule;
  RKH_TRY(launch_edges(p, grid, 0, p->d_io_probe, nullptr, auto_steer_plan(p, grid, 0, false)));
  hipLaunchKernelGGL(probes_flushed_kernel, dim3(p->P), dim3(64), 0, p->stream, p->d_probs);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// the timing events [2 slot] and [2 slot + 1] of a profiled round exist
rkh_status ensure_event_pair(std::vector<hipEvent_t>& ev, uint32_t slot) {
  while (ev.size() < 2 * size_t(slot + 1)) {
    hipEvent_t e;
    RKH_HIP(hipEventCreate(&e));
    ev.push_back(e);
  }
  return RKH_OK;
}

// round_begin_kernel's arguments for the round in profile slot `slot`; plan: the round's steer plan
RoundBeginArgs round_begin_args(const rkh_planner* p, uint32_t slot, bool fit, const SteerPlan& plan) {
  RoundBeginArgs a;
  a.probs = p->d_probs;
  a.P = p->P;
  a.round_slot = slot;
  a.sel = p->d_sel;
  a.parity = p->round_parity;
  a.fit_fill = fit ? float(p->wave_fill) : 0.0f;
  a.slots = p->wave_slots;
  a.wave_base = p->d_wave_base;
  a.edge_base = p->d_edge_base;
  a.nn_base = p->d_nn_base;
  a.nn_queries = p->nn_mirror ? nn1_mirror_queries() : nn1_mfma_queries();
  a.epw = pair_kernel_edges_per_wave();
  a.step_cnt = p->d_step_cnt;
  a.carry_fit_lo = p->carry_fit ? plan.carry_lo : kCarryOff;
  return a;
}

rkh_status enqueue_round(rkh_planner* p) {
  hipStream_t s = p->stream;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t slot = 0;
  if (p->profile_nn && p->prof_rounds < rkh_planner::kProfMax) {
    slot = p->prof_rounds++;
    RKH_TRY(ensure_event_pair(p->ev, slot));
    ev0 = p->ev[2 * slot];
    ev1 = p->ev[2 * slot + 1];
    RKH_TRY(ensure_event_pair(p->ev_steer, slot));
  }
  // the round's batch scale is chosen on the device (round_begin_kernel); the launches are sized for its upper end
  const bool fit = p->wave_fit && p->steer == SteerMapping::Auto;
  const float scale = fit ? kFitScaleHi : 1.0f;
  // launch sizes of this round from the host-side bounds
  uint32_t batch_ub = 1;
  p->prev_sum_batch_ub = p->sum_batch_ub ? p->sum_batch_ub : uint64_t(p->b_max) * p->P;
  p->sum_batch_ub = 0;
  p->max_n_ub = 1;
  for (uint32_t i = 0; i < p->P; ++i) {
    const PlannerState& hs = p->prob[i].h_state;
    const uint32_t b = batch_upper_bound(hs, p->n_ub[i], scale);
    batch_ub = std::max(batch_ub, b);
    p->sum_batch_ub += b;
    p->max_n_ub = std::max(p->max_n_ub, p->n_ub[i]);
    p->n_ub[i] = std::min<uint64_t>(p->n_ub[i] + b, uint64_t(hs.max_total));
  }
  const uint32_t probe_ub = p->prev_batch_ub ? p->prev_batch_ub : p->b_max;
  p->prev_batch_ub = batch_ub + kProbeGranule;  // next round's probes: this round's vertices + what was left over
  p->round_parity ^= 1u;
  const SteerPlan plan = auto_steer_plan(p, batch_ub, probe_ub, true);
  hipLaunchKernelGGL(round_begin_kernel, dim3(1), dim3(256), 0, s, round_begin_args(p, slot, fit, plan));
  // 1. NN sweep of every problem's samples over its snapshot
  rkh_status st = p->nn_mirror
                      ? launch_nn1_mirror(s, p->D, p->d_nn_args, p->P, p->max_n_ub, batch_ub, p->x_norm_bound, p->mirror_scale,
                                          p->d_nn_base, p->nn_open, ev0, ev1)
                      : launch_nn1(s, p->D, NnArgs(), p->d_nn_args, p->P, p->max_capacity, batch_ub, p->part_blocks, ev0,
                                   ev1, p->coord_bound, p->d_nn_base, true);
  if (st != RKH_OK) return st;
  // 2. speculative steer of all candidates + the goal probes of the vertices the previous round committed
  if (ev0) (void)hipEventRecord(p->ev_steer[2 * slot], s);
  st = launch_edges(p, batch_ub, probe_ub, p->d_io_steer, p->d_io_probe, plan);
  if (st != RKH_OK) return st;
  if (ev0) (void)hipEventRecord(p->ev_steer[2 * slot + 1], s);
  // 3. fix-up against the vertices this round itself would add
  RKH_TRY(launch_fixup(p, batch_ub));
  // 4. commit the valid prefix
  ProbeReachDev reach = p->reach;
  reach.round_edges = p->d_sel + p->round_parity;  // this round's edges; the next round's begin clears the other word
  hipLaunchKernelGGL(commit_kernel, dim3(p->P), dim3(256), 0, s, p->d_probs, p->D, p->DP, fit ? kProbeGranule : 1u,
                     p->carry, reach);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// ---- the device tables: entry i of each as a function of problem i ----------------------------------------------------
ProblemDev problem_dev(const rkh_planner* p, uint32_t i) {
  const Problem& q = p->prob[i];
  ProblemDev pd;
  pd.st = p->d_states + i;
  pd.tree = q.d_tree;
  pd.parent = q.d_parent;
  pd.node_sample = q.d_node_sample;
  pd.samples = q.d_samples;
  pd.nn_seq = q.d_nn_seq;
  pd.accept_log = q.d_accept_log;
  pd.nn_idx = q.d_nn_idx;
  pd.nn_dist = q.d_nn_dist;
  pd.x_out = q.d_x_out;
  pd.accept = q.d_accept;
  pd.steps = q.d_steps;
  pd.stash_x = q.d_stash_x;
  pd.stash_nn = q.d_stash_nn;
  pd.stash_steps = q.d_stash_steps;
  pd.stash_accept = q.d_stash_accept;
  pd.round_n = q.d_round_n;
  pd.mirror = static_cast<uint4*>(q.d_mirror);
  pd.dx_max_bits = q.dx_max_bits;
  pd.mirror_scale = p->mirror_scale;
  pd.goal = q.d_goal;
  pd.goal_dist = q.d_goal_dist;
  pd.probe_list = q.d_probe_list;
  return pd;
}

NnArgs nn_args(const rkh_planner* p, uint32_t i) {
  const Problem& q = p->prob[i];
  PlannerState* st = p->d_states + i;
  NnArgs na;
  na.pos = q.d_tree;
  na.d_n = &st->n;
  na.q = q.d_samples;
  na.d_qoff = &st->s0;
  na.B = p->b_max;
  na.d_B = &st->B;
  na.part_dist = q.d_part_dist;
  na.part_idx = q.d_part_idx;
  na.seed = q.d_part_idx + uint64_t(p->part_blocks) * p->b_max;
  na.idx = q.d_nn_idx;
  na.dist = q.d_nn_dist;
  na.mirror = q.d_mirror;
  if (q.d_cand) {
    nn1_mirror_carve(q.d_cand, p->b_max, &na);
    na.dx_max_bits = q.dx_max_bits;
  }
  return na;
}

EdgeIO steer_io(const rkh_planner* p, uint32_t i) {
  const Problem& q = p->prob[i];
  PlannerState* st = p->d_states + i;
  EdgeIO io;
  io.src = q.d_tree;
  io.src_idx = q.d_nn_idx;
  io.src_stride = p->DP;
  io.tgt = q.d_samples;
  io.d_tgt_off = &st->s0;
  io.tgt_stride = p->D;
  io.B = p->b_max;
  io.d_B = &st->B;
  io.x_out = q.d_x_out;
  io.steps_free = q.d_steps;
  io.mode = EDGE_STEER_ACCEPT;
  io.best_case = q.d_nn_dist;
  io.steer_tol = q.prm.steer_tol;
  io.accept = q.d_accept;
  io.err_flag = p->scene->d_err.get();
  return io;
}

EdgeIO probe_io(const rkh_planner* p, uint32_t i) {
  const Problem& q = p->prob[i];
  PlannerState* st = p->d_states + i;
  EdgeIO gp;
  gp.src = q.d_tree;
  gp.src_idx = q.d_probe_list;  // edge e = the e-th open probe; edge_source_row / pair_edge_rows of every steer form
  gp.src_stride = p->DP;
  gp.tgt = q.d_goal;
  gp.tgt_stride = 0;
  gp.B = p->b_max + kProbeGranule;
  gp.d_B = &st->n_new;
  gp.x_out = q.d_probe_x;
  gp.steps_free = q.d_probe_steps;
  gp.mode = EDGE_GOAL_PROBE;
  gp.goal_dist = q.d_goal_dist;
  gp.err_flag = p->scene->d_err.get();
  return gp;
}

// generate_rrt has no iteration cap (rr_tree.hpp:192-196: keep_going() looks at the vertex count only), so the device-
// resident sample stream and its per-iteration logs must not have one either: when a problem's cursor comes near the
// end of its buffers they are re-allocated at twice the size: buffers of their own, which supersede the ranges of the
// arena the problem started in.  Called with both streams idle (rkh_planner_sync).  A failure before the swap leaves the
// problem as it was.
rkh_status grow_sample_buffers(rkh_planner* p, uint32_t i, uint64_t new_cap) {
  Problem& q = p->prob[i];
  const int D = p->D;
  DeviceBuffer<double> ns;
  DeviceBuffer<uint32_t> nq;
  DeviceBuffer<uint8_t> na;
  RKH_TRY(ns.alloc(new_cap * D));
  RKH_TRY(nq.alloc(new_cap));
  RKH_TRY(na.alloc(new_cap));
  RKH_HIP(hipMemcpy(ns.get(), q.d_samples, q.samples_ready * D * sizeof(double), hipMemcpyDeviceToDevice));
  RKH_HIP(hipMemcpy(nq.get(), q.d_nn_seq, q.sample_cap * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  RKH_HIP(hipMemcpy(na.get(), q.d_accept_log, q.sample_cap, hipMemcpyDeviceToDevice));
  q.grown_samples = std::move(ns);  // (frees the ones of an earlier growth; the arena's first ranges just lie idle)
  q.grown_nn_seq = std::move(nq);
  q.grown_accept_log = std::move(na);
  q.d_samples = q.grown_samples.get();
  q.d_nn_seq = q.grown_nn_seq.get();
  q.d_accept_log = q.grown_accept_log.get();
  q.sample_cap = new_cap;
  // the device tables that point into these buffers
  const double* cs = q.d_samples;
  uint32_t* cq = q.d_nn_seq;
  uint8_t* ca = q.d_accept_log;
  RKH_HIP(hipMemcpy(&p->d_probs[i].samples, &cs, sizeof(cs), hipMemcpyHostToDevice));
  RKH_HIP(hipMemcpy(&p->d_probs[i].nn_seq, &cq, sizeof(cq), hipMemcpyHostToDevice));
  RKH_HIP(hipMemcpy(&p->d_probs[i].accept_log, &ca, sizeof(ca), hipMemcpyHostToDevice));
  RKH_HIP(hipMemcpy(&p->d_nn_args[i].q, &cs, sizeof(cs), hipMemcpyHostToDevice));
  RKH_HIP(hipMemcpy(&p->d_io_steer[i].tgt, &cs, sizeof(cs), hipMemcpyHostToDevice));
  return RKH_OK;
}

// The states of all problems and the scene's error flag (*p->h_err), read into the pinned block: two copies queued back
// to back, one wait.
rkh_status read_states(rkh_planner* p) {
  PlannerState* hs = reinterpret_cast<PlannerState*>(p->h_block.get() + p->layout.shared[SR_STATES].off);
  RKH_HIP(hipMemcpyAsync(hs, p->d_states, p->P * sizeof(PlannerState), hipMemcpyDeviceToHost, p->stream));
  RKH_HIP(hipMemcpyAsync(p->h_err, p->scene->d_err.get(), sizeof(int), hipMemcpyDeviceToHost, p->stream));
  RKH_HIP(hipStreamSynchronize(p->stream));
  for (uint32_t i = 0; i < p->P; ++i) {
    p->prob[i].h_state = hs[i];
    p->n_ub[i] = hs[i].n;  // the stream is idle: the bound is exact again
  }
  uint32_t pending = 1;
  for (uint32_t i = 0; i < p->P; ++i) pending = std::max(pending, hs[i].n_new);
  p->prev_batch_ub = pending;
  return RKH_OK;
}

// ---- rkh_planner_create*: the phases, in the order they run -----------------------------------------------------------

// 1. What the arguments alone decide; nothing exists yet.
rkh_status check_create_args(const rkh_scene* scene, const rkh_dyn_space* space, const rkh_qs_space* qspace,
                             const rkh_rrt_params* prms, uint32_t n_problems, rkh_planner** out) {
  if (!scene || (!space && !qspace) || !prms || !out || n_problems < 1) return RKH_ERR_BAD_ARG;
  const int space_dof = space ? space->n_dof : qspace->n_dof;
  if (space_dof != scene->host.n_dof) {
    set_error("rkh_planner_create: the space's n_dof does not match the scene");
    return RKH_ERR_BAD_ARG;
  }
  for (uint32_t i = 0; i < n_problems; ++i)
    if (prms[i].max_vertices < 1) {
      set_error("rkh_planner_create: max_vertices < 1");
      return RKH_ERR_BAD_ARG;
    }
  if (qspace && (!(qspace->min_interval > 0.0) || qspace->n_dof > kMaxDof)) {
    set_error("rkh_qs_space: min_interval must be positive");
    return RKH_ERR_BAD_ARG;
  }
  return RKH_OK;
}

// 2. The space: dimensions, the sampled hyperbox, the device form of the space, and the two bounds the NN sweeps take
// from the largest |coordinate| per dimension.
rkh_status setup_space(rkh_planner* p, const rkh_dyn_space* space, const rkh_qs_space* qspace, const rkh_rrt_params* prms) {
  if (space) {
    p->D = 2 * space->n_dof;
    for (int d = 0; d < p->D; ++d) {
      p->lower[d] = space->lower[d];
      p->upper[d] = space->upper[d];
    }
    RKH_TRY(build_dyn_dev(*space, 1.0, &p->dyn));
  } else {
    p->quasi_static = true;
    p->D = qspace->n_dof;
    std::memset(&p->qs, 0, sizeof(p->qs));
    p->qs.min_interval = qspace->min_interval;
    p->qs.fraction = 1.0;
    qs_set_speed(p->qs, qspace->speed_limits, qspace->n_dof);
    for (int d = 0; d < p->D; ++d) {
      p->lower[d] = p->qs.lower[d] = qspace->lower[d];
      p->upper[d] = p->qs.upper[d] = qspace->upper[d];
    }
  }
  p->DP = nn_padded_dims(p->D);
  // vertices and samples lie inside the hyperbox (is_free / random_point), and the roots are vertices too: the bound of
  // the NN sweep's float pre-filter, and the norm bound of the mirror sweep
  for (int d = 0; d < p->D; ++d) {
    double m = std::max(std::fabs(p->lower[d]), std::fabs(p->upper[d]));
    for (uint32_t i = 0; i < p->P; ++i) m = std::max(m, std::fabs(prms[i].start[d]));
    p->coord_bound = std::max(p->coord_bound, m);
    p->x_norm_bound += m * m;
  }
  p->x_norm_bound = std::sqrt(p->x_norm_bound) * (1.0 + 1e-9);
  p->nn_mirror = nn1_mirror_applies(p->D, p->coord_bound);
  if (p->nn_mirror) p->mirror_scale = mirror_prescale(p->coord_bound);
  return RKH_OK;
}

// 3. Tuning: every environment knob, the steer plan and the batch rule.  Writes into the planner, allocates nothing.
void tune_planner(rkh_planner* p, const rkh_rrt_params* prms) {
  const rkh_scene* scene = p->scene;
  if (const char* e = getenv("RKH_WAVE_FIT")) p->wave_fit = atoi(e);
  if (const char* e = getenv("RKH_WAVE_FILL")) p->wave_fill = atof(e);
  // Many problems per planner: a round's candidates per problem stay within ONE query block of the mirror sweep (a
  // second block re-reads the whole tree for a handful of queries; 512 problems x 100 000: 7.45 -> 7.62 M expansions/s).
  // The batch rule only reaches the cap late in a run (1.25 sqrt(n) = 384 at n = 94 k) or through the wave fit's scale.
  if (p->nn_mirror && p->P >= 64) p->b_max = std::min(p->b_max, nn1_mirror_queries());
  if (const char* e = getenv("RKH_BATCH_MAX")) p->b_max = std::max(8, atoi(e));
  p->b_max = std::min<uint32_t>(p->b_max, 4096);
  if (const char* e = getenv("RKH_LANE_THRESHOLD")) p->lane_threshold = uint32_t(std::max(0, atoi(e)));
  if (!p->quasi_static) {
    const SteerRequest req = steer_request();
    p->steer = steer_mapping(scene->host, SteerEntry::BatchPlanner, req, 0, p->P, p->b_max);
    note_steer_mapping(p->steer);
    p->duo_threshold = req.duo_threshold;
    p->steer_clearance = req.clearance;
  }
  if (p->lane_kernel()) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, scene->ctx->device) == hipSuccess && prop.multiProcessorCount > 0)
      p->wave_slots = uint32_t(prop.multiProcessorCount) * pair_kernel_waves_per_cu(scene->host.n_dof, scene->host.has_prismatic != 0);
    if (getenv("RKH_VERBOSE")) fprintf(stderr, "rkh planner: %d CUs, %u resident steer waves\n", prop.multiProcessorCount, p->wave_slots);
  }
  p->split_min_edges = p->wave_slots / 2 * pair_kernel_edges_per_wave();
  if (const char* e = getenv("RKH_STEER_SPLIT_MIN_EDGES")) p->split_min_edges = uint32_t(std::max(0, atoi(e)));
  p->step_blocks_cap = 2 * p->wave_slots;
  if (p->lane_kernel()) {
    // the step kernel's blocks take their RK4 workspace out of the two-lanes workspace
    const size_t lane_ws = propagate_pairs_workspace_bytes(p->n_dof, p->b_max, p->b_max, p->P);
    if (propagate_pair_step_workspace_bytes(p->n_dof, p->step_blocks_cap) > lane_ws)
      p->step_blocks_cap = uint32_t(lane_ws / propagate_pair_step_workspace_bytes(p->n_dof, 1));
  }
  p->carry = !p->quasi_static && p->steer == SteerMapping::Auto && p->dyn.n_steps > 1;
  if (const char* e = getenv("RKH_STEER_CARRY")) p->carry = p->carry && atoi(e) != 0;
  p->carry_min_edges = p->wave_slots / 2 * pair_kernel_edges_per_wave();
  if (const char* e = getenv("RKH_STEER_CARRY_MIN_EDGES")) p->carry_min_edges = uint32_t(std::max(0, atoi(e)));
  if (const char* e = getenv("RKH_STEER_CARRY_FIT")) p->carry_fit = atoi(e) != 0;
  if (const char* e = getenv("RKH_PROFILE_NN")) p->profile_nn = atoi(e) != 0;
  p->nn_open = nn1_mirror_open_lists();
  if (const char* e = getenv("RKH_FIXUP_TILED")) p->fixup_tiled = atoi(e) != 0;
  // candidates per round = batch_factor * sqrt(n) per problem (results do not depend on it).  More candidates per
  // round mean fewer rounds but more discarded speculation (0.89 of the propagated edges are committed at 1.25, 0.72 at
  // 2, 0.55 at 3, 0.45 at 4), and a round is only cheap to enlarge while the chip is not full.  Measured optimum
  // (tests/diag_bench_sweep.sh, tests/diag_single.py): 1.25 for 256 problems x 100 000 vertices (5.6 M expansions/s),
  // 2 for 32 ... 128 problems (64 x 100 000: 3.03 M against 2.86 at 1.25 and 2.51 at 4), 4 for 16 (444 k against 322 k
  // at 1.25), 2 = 4 for a single problem (bound by the latency of one edge; 2 checks fewer edges).  The rule: what
  // brings a mid-run round (n = max_vertices / 2) of all problems to ~32 k edges -- one 32-edge steer wave per SIMD --
  // within [1.25, 2], up to 4 for at most 16 problems.
  double mid_sqrt_sum = 0.0;
  for (uint32_t i = 0; i < p->P; ++i) mid_sqrt_sum += std::sqrt(0.5 * double(prms[i].max_vertices));
  const double factor_cap = p->P == 1 ? 2.0 : (p->P <= 16 ? 4.0 : 2.0);
  p->batch_factor = float(std::min(factor_cap, std::max(1.25, 32768.0 / mid_sqrt_sum)));
  if (const char* e = getenv("RKH_BATCH_FACTOR")) p->batch_factor = float(atof(e));
  if (const char* e = getenv("RKH_BATCH_MIN")) p->b_min = std::max(1, atoi(e));
  if (const char* e = getenv("RKH_SAMPLE_CAP")) p->sample_cap_min = strtoull(e, nullptr, 10);
  if (const char* e = getenv("RKH_ARENA_CACHE")) p->arena_cache = atoi(e) != 0;
  if (const char* e = getenv("RKH_ARENA_POISON")) p->arena_poison = atoi(e) != 0;
}

// 3b. The travel bound of a steered edge of this scene and space (probe_reach.h), from the scene's host chain and the
// space's device form; +inf wherever probe_travel gives no certificate.
static_assert(kMaxDof <= kReachMaxDof, "probe_reach.h holds a chain of kMaxDof joints");
void setup_probe_reach(rkh_planner* p) {
  ProbeReachDev& r = p->reach;
  r.reach_q = INFINITY;
  r.round_edges = nullptr;  // (set per round, enqueue_round)
  // rounds that fill the chip: the default of carry_min_edges (RKH_PROBE_REACH_MIN_EDGES overrides it)
  r.min_edges = p->wave_slots / 2 * pair_kernel_edges_per_wave();
  if (const char* e = getenv("RKH_PROBE_REACH_MIN_EDGES")) r.min_edges = uint32_t(std::max(0, atoi(e)));
  for (int j = 0; j < kReachMaxDof; ++j) r.v_lower[j] = r.v_upper[j] = 0.0;
  if (p->quasi_static) return;
  if (const char* e = getenv("RKH_PROBE_REACH"))
    if (atoi(e) == 0) return;
  const SceneDev& S = p->scene->host;
  ReachChain c;
  c.n_dof = S.n_dof;
  c.serial = S.n_branches == 0 && S.planar == 0;
  c.all_revolute = S.prismatic_mask == 0u;
  c.beam = S.beam_on != 0;
  for (int k = 0; k < 3; ++k) c.base_acc[k] = S.base_acc[k];
  for (int j = 0; j < S.n_dof && j < kReachMaxDof; ++j) {
    const JointDev& J = S.joints[j];
    ReachJoint& o = c.joints[j];
    for (int k = 0; k < 3; ++k) {
      o.axis[k] = J.axis[k];
      o.off_pos[k] = J.off_pos[k];
    }
    o.joint_inertia = J.joint_inertia;
    o.mass = J.mass;
    for (int k = 0; k < 6; ++k) o.inertia[k] = J.inertia[k];
  }
  ReachDyn d;
  d.n_dof = p->n_dof;
  d.n_steps = p->dyn.n_steps;
  d.dt = p->dyn.dt;
  d.u_max = p->dyn.u_max;
  d.single_inner = true;
  for (int k = 0; k < p->dyn.n_steps; ++k) d.single_inner = d.single_inner && p->dyn.inner[k] == 1;
  for (int j = 0; j < p->n_dof; ++j) {  // state layout (q0, qd0, q1, qd1, ...)
    d.v_lower[j] = r.v_lower[j] = p->dyn.lower[2 * j + 1];
    d.v_upper[j] = r.v_upper[j] = p->dyn.upper[2 * j + 1];
  }
  double T[kReachMaxDof];
  if (probe_travel(c, d, T)) r.reach_q = probe_reach_norm(T, c.n_dof);
  if (getenv("RKH_VERBOSE")) fprintf(stderr, "rkh planner: goal-probe reach %g rad\n", r.reach_q);
}

// 4. The streams, then the memory: the arena's layout from the shape of the batch, the slab itself -- one the context
// kept from an earlier planner, or a new one -- and every device pointer of the planner set to its range; the pinned
// block beside it.
rkh_status alloc_planner_buffers(rkh_planner* p) {
  const uint32_t P = p->P, b_max = p->b_max;
  RKH_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  RKH_HIP(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
  std::vector<uint64_t> capacity(P), sample_cap(P), mirror_bytes(P);
  for (uint32_t i = 0; i < P; ++i) {
    Problem& q = p->prob[i];
    q.sample_cap = planner_sample_cap(q.prm.max_vertices, b_max, p->sample_cap_min);
    capacity[i] = q.capacity;
    sample_cap[i] = q.sample_cap;
    mirror_bytes[i] = nn1_mirror_bytes(q.capacity);
  }
  ArenaShape sh;
  sh.P = P;
  sh.capacity = capacity.data();
  sh.sample_cap = sample_cap.data();
  sh.mirror_bytes = mirror_bytes.data();
  sh.b_max = b_max;
  sh.probe_granule = kProbeGranule;
  sh.part_blocks = p->part_blocks;
  sh.prof_rounds = rkh_planner::kProfMax;
  sh.D = p->D;
  sh.DP = p->DP;
  sh.mirror = p->nn_mirror;
  sh.profile = p->profile_nn;
  sh.lane = p->lane_kernel();
  sh.carry = p->carry;
  sh.cand_bytes = nn1_mirror_query_bytes() * b_max + 256;  // the per-query scratch, then the mirror's error word
  if (sh.lane) {
    // (sized for the largest grid of a launch: b_max candidates and up to b_max + kProbeGranule goal probes per problem,
    // see prev_batch_ub and flush_probes)
    sh.lane_ws_bytes = propagate_pairs_workspace_bytes(p->n_dof, b_max, b_max + kProbeGranule, P);
    p->step_list_cap = P * (2 * b_max + kProbeGranule);
    sh.step_list_bytes = size_t(p->step_list_cap) * sizeof(uint4);
  }
  sh.state_bytes = sizeof(PlannerState);
  sh.prob_bytes = sizeof(ProblemDev);
  sh.nn_args_bytes = sizeof(NnArgs);
  sh.edge_io_bytes = sizeof(EdgeIO);
  sh.init_bytes = sizeof(ProblemInit);
  sh.sample_seg_bytes = sizeof(SampleSeg);
  sh.goal_seg_bytes = sizeof(GoalSeg);
  sh.max_steps = kMaxSteps;
  p->layout = planner_arena_layout(sh);
  const ArenaLayout& L = p->layout;
  RKH_TRY(ctx_take_arena(p->ctx, L.total, p->arena_cache, &p->arena));
  const DeviceArena& A = p->arena;
  // diagnostic: nothing may depend on what the memory held before, zeroes included
  if (p->arena_poison) RKH_HIP(hipMemsetAsync(A.get(), 0xA5, A.size(), p->stream));
  p->d_bounds = A.at<double>(L.shared[SR_BOUNDS]);
  p->d_states = A.at<PlannerState>(L.shared[SR_STATES]);
  p->d_probs = A.at<ProblemDev>(L.shared[SR_PROBS]);
  p->d_nn_args = A.at<NnArgs>(L.shared[SR_NN_ARGS]);
  p->d_io_steer = A.at<EdgeIO>(L.shared[SR_IO_STEER]);
  p->d_io_probe = A.at<EdgeIO>(L.shared[SR_IO_PROBE]);
  p->d_wave_base = A.at<uint32_t>(L.shared[SR_WAVE_BASE]);
  p->d_edge_base = p->d_wave_base ? p->d_wave_base + (2 * P + 1) : nullptr;
  p->d_step_cnt = A.at<uint32_t>(L.shared[SR_STEP_CNT]);
  p->d_nn_base = A.at<uint32_t>(L.shared[SR_NN_BASE]);
  p->d_sel = A.at<uint32_t>(L.shared[SR_SEL]);
  p->d_steps_exec = A.at<unsigned long long>(L.shared[SR_STEPS_EXEC]);
  p->staging[0].d_tab = A.at<SampleSeg>(L.shared[SR_SAMPLE_TAB0]);
  p->staging[1].d_tab = A.at<SampleSeg>(L.shared[SR_SAMPLE_TAB1]);
  p->d_gd_tab = A.at<GoalSeg>(L.shared[SR_GOAL_TAB]);
  p->d_lane_ws = A.at<double>(L.shared[SR_LANE_WS]);
  p->d_step_list[0] = A.at<uint4>(L.shared[SR_STEP_LIST0]);
  p->d_step_list[1] = A.at<uint4>(L.shared[SR_STEP_LIST1]);
  for (uint32_t i = 0; i < P; ++i) {
    Problem& q = p->prob[i];
    q.d_mt = A.at<uint32_t>(L.of(i, PR_MT));
    q.d_tree = A.at<double>(L.of(i, PR_TREE));
    q.d_parent = A.at<uint32_t>(L.of(i, PR_PARENT));
    q.d_node_sample = A.at<uint32_t>(L.of(i, PR_NODE_SAMPLE));
    q.d_goal_dist = A.at<double>(L.of(i, PR_GOAL_DIST));
    q.d_samples = A.at<double>(L.of(i, PR_SAMPLES));
    q.d_nn_seq = A.at<uint32_t>(L.of(i, PR_NN_SEQ));
    q.d_accept_log = A.at<uint8_t>(L.of(i, PR_ACCEPT_LOG));
    q.d_nn_idx = A.at<uint32_t>(L.of(i, PR_NN_IDX));
    q.d_nn_dist = A.at<double>(L.of(i, PR_NN_DIST));
    q.d_x_out = A.at<double>(L.of(i, PR_X_OUT));
    q.d_steps = A.at<uint32_t>(L.of(i, PR_STEPS));
    q.d_accept = A.at<uint8_t>(L.of(i, PR_ACCEPT));
    q.d_probe_x = A.at<double>(L.of(i, PR_PROBE_X));
    q.d_probe_steps = A.at<uint32_t>(L.of(i, PR_PROBE_STEPS));
    q.d_probe_list = A.at<uint32_t>(L.of(i, PR_PROBE_LIST));
    q.d_goal = A.at<double>(L.of(i, PR_GOAL));
    q.d_part_dist = A.at<double>(L.of(i, PR_PART_DIST));
    q.d_part_idx = A.at<uint32_t>(L.of(i, PR_PART_IDX));
    q.d_round_n = A.at<uint32_t>(L.of(i, PR_ROUND_N));
    q.d_mirror = A.at<void>(L.of(i, PR_MIRROR));
    q.d_cand = A.at<void>(L.of(i, PR_CAND));
    q.d_stash_x = A.at<double>(L.of(i, PR_STASH_X));
    q.d_stash_nn = A.at<uint32_t>(L.of(i, PR_STASH_NN));
    q.d_stash_steps = A.at<uint32_t>(L.of(i, PR_STASH_STEPS));
    q.d_stash_accept = A.at<uint8_t>(L.of(i, PR_STASH_ACCEPT));
    q.dx_max_bits = q.d_cand ? reinterpret_cast<uint32_t*>(static_cast<char*>(q.d_cand) + nn1_mirror_query_bytes() * b_max) : nullptr;
  }
  // the pinned block: image of the upload ranges | error flag | segment tables
  const size_t seg_tab = arena_align_up(P * sizeof(SampleSeg)), gd_tab = arena_align_up(P * sizeof(GoalSeg));
  RKH_TRY(p->h_block.alloc(L.upload_bytes + kArenaAlign + 2 * seg_tab + gd_tab));
  char* h = p->h_block.get() + L.upload_bytes;
  p->h_err = reinterpret_cast<int*>(h);
  p->staging[0].h_tab = reinterpret_cast<SampleSeg*>(h + kArenaAlign);
  p->staging[1].h_tab = reinterpret_cast<SampleSeg*>(h + kArenaAlign + seg_tab);
  p->h_gd_tab = reinterpret_cast<GoalSeg*>(h + kArenaAlign + 2 * seg_tab);
  return RKH_OK;
}

// 5. The image of the upload ranges, in the pinned block: the sampled box, every problem's initial device state and its
// entry in the five tables, its row of the init table, and the zeroes of the round counters and prefixes.
void fill_upload_image(rkh_planner* p) {
  const ArenaLayout& L = p->layout;
  char* h = p->h_block.get();
  std::memset(h, 0, L.upload_bytes);
  auto image = [&](SharedRange r) { return h + L.shared[r].off; };
  double* bounds = reinterpret_cast<double*>(image(SR_BOUNDS));
  for (int d = 0; d < p->D; ++d) {
    bounds[d] = p->lower[d];
    bounds[p->D + d] = p->upper[d];
  }
  PlannerState* hs = reinterpret_cast<PlannerState*>(image(SR_STATES));
  ProblemDev* hp = reinterpret_cast<ProblemDev*>(image(SR_PROBS));
  NnArgs* hn = reinterpret_cast<NnArgs*>(image(SR_NN_ARGS));
  EdgeIO* hio = reinterpret_cast<EdgeIO*>(image(SR_IO_STEER));
  EdgeIO* hgp = reinterpret_cast<EdgeIO*>(image(SR_IO_PROBE));
  ProblemInit* hi = reinterpret_cast<ProblemInit*>(image(SR_INIT_TAB));
  for (uint32_t i = 0; i < p->P; ++i) {
    Problem& q = p->prob[i];
    PlannerState& s0 = q.h_state;
    std::memset(&s0, 0, sizeof(s0));
    s0.n = 1;  // root vertex = query start (create_root, rrt_path_planner.tpp:131-133)
    s0.probed_n = 1;  // (the list of open probes is empty: list_n = n_new = 0)
    s0.max_total = uint32_t(q.prm.max_vertices) + 1;
    s0.b_max = p->b_max;
    s0.b_min = p->b_min;
    s0.batch_factor = p->batch_factor;
    hs[i] = s0;
    hp[i] = problem_dev(p, i);
    hn[i] = nn_args(p, i);
    hio[i] = steer_io(p, i);
    hgp[i] = probe_io(p, i);
    ProblemInit& pi = hi[i];
    pi.mt = q.d_mt;
    pi.tree = q.d_tree;
    pi.parent = q.d_parent;
    pi.goal = q.d_goal;
    pi.seed_row = q.d_part_idx + uint64_t(p->part_blocks) * p->b_max;
    pi.cand = static_cast<uint32_t*>(q.d_cand);
    pi.mirror = static_cast<uint4*>(q.d_mirror);
    pi.dx_max_bits = q.dx_max_bits;
    pi.mirror_frags = q.d_mirror ? nn1_mirror_bytes(q.capacity) / sizeof(uint4) : 0;
    pi.mirror_scale = p->mirror_scale;
    pi.seed = uint32_t(q.prm.seed);
    for (int d = 0; d < p->D; ++d) {
      pi.start[d] = q.prm.start[d];
      pi.goal_x[d] = q.prm.goal[d];
    }
  }
}

// 6. One copy for the upload ranges, then the init pass over all problems (mirror_fill_all_kernel, planner_init_kernel).
// Returns with the stream idle: an error of the pass is create's error.
rkh_status init_device(rkh_planner* p) {
  const ArenaLayout& L = p->layout;
  RKH_HIP(hipMemcpyAsync(p->arena.get(), p->h_block.get(), L.upload_bytes, hipMemcpyHostToDevice, p->stream));
  const ProblemInit* d_init = p->arena.at<ProblemInit>(L.shared[SR_INIT_TAB]);
  if (p->nn_mirror) {
    const uint64_t max_frags = nn1_mirror_bytes(p->max_capacity) / sizeof(uint4);
    const uint32_t gx = uint32_t(std::min<uint64_t>(std::max<uint64_t>((max_frags + 1023) / 1024, 1), 65535));
    hipLaunchKernelGGL(mirror_fill_all_kernel, dim3(gx, p->P), dim3(256), 0, p->stream, d_init);
  }
  const uint32_t cand_words = p->nn_mirror ? uint32_t((nn1_mirror_query_bytes() * p->b_max + 256) / sizeof(uint32_t)) : 0u;
  hipLaunchKernelGGL(planner_init_kernel, dim3(p->P), dim3(256), 0, p->stream, d_init, p->D, p->DP, p->b_max, cand_words);
  RKH_HIP(hipGetLastError());
  RKH_HIP(hipStreamSynchronize(p->stream));
  return RKH_OK;
}

rkh_status planner_create_common(rkh_scene* scene, const rkh_dyn_space* space, const rkh_qs_space* qspace,
                                 const rkh_rrt_params* prms, uint32_t n_problems, rkh_planner** out) {
  RKH_TRY(check_create_args(scene, space, qspace, prms, n_problems, out));
  std::unique_ptr<rkh_planner> p(new rkh_planner());  // the caller's only once the last step has succeeded
  p->scene = scene;
  p->ctx = scene->ctx;
  p->n_dof = scene->host.n_dof;
  p->P = n_problems;
  RKH_TRY(setup_space(p.get(), space, qspace, prms));
  RKH_HIP(hipSetDevice(scene->ctx->device));  // (before the tuning: its occupancy query acts on the current device)
  tune_planner(p.get(), prms);
  setup_probe_reach(p.get());
  p->prob.resize(n_problems);
  for (uint32_t i = 0; i < n_problems; ++i) {
    Problem& q = p->prob[i];
    q.prm = prms[i];
    q.capacity = planner_capacity_rows(prms[i].max_vertices);
    p->max_capacity = std::max(p->max_capacity, q.capacity);
  }
  p->part_blocks = nn1_partial_blocks(p->D, p->max_capacity, p->b_max, n_problems, p->coord_bound);
  p->n_ub.assign(n_problems, 1);
  RKH_TRY(alloc_planner_buffers(p.get()));
  fill_upload_image(p.get());
  RKH_TRY(init_device(p.get()));
  *out = p.release();
  return RKH_OK;
}

// ---- rkh_planner_sync: the three steps --------------------------------------------------------------------------------

// 1. The states of all problems and the scene's error flag; a finished batch first runs the goal probes of its last
// committed vertices.
rkh_status read_round_results(rkh_planner* p) {
  RKH_TRY(read_states(p));
  const int flag = *p->h_err;
  if (flag != 0) {
    RKH_HIP(hipMemset(p->scene->d_err.get(), 0, sizeof(int)));
    set_error("planner: mass matrix is singular (Cholesky pivot < 1e-8)");
    return rkh_status(flag);
  }
  bool all_done = true, pending = false;
  for (Problem& q : p->prob) {
    if (!(q.truncated || q.h_state.done == 1)) all_done = false;
    if (q.h_state.probed_n < q.h_state.n) pending = true;
  }
  if (all_done && pending) {  // finished: run the goal probes of the last committed vertices
    RKH_TRY(flush_probes(p));
    RKH_TRY(read_states(p));
  }
  return RKH_OK;
}

// Goal-probe results of problem q that no sync has looked at yet: vertices [1, probed_n) have one, the first
// goal_checked of them are done (a truncated problem takes no more).
uint64_t new_goal_probes(const Problem& q) {
  const uint64_t probed = q.h_state.probed_n < 1 ? 1 : q.h_state.probed_n;
  return (!q.truncated && probed > 1 && q.goal_checked < probed - 1) ? probed - 1 - q.goal_checked : 0;
}

// 2. The new goal-probe results of all problems: gathered on the device, one copy into the pinned buffer, one wait.
// Problem i's gd_cnt[i] results start at h_gd[gd_off[i]].  probed_n jumps to n wherever commit_kernel settled every new
// vertex, so one sync may take all of a problem's vertices since the last one: both buffers are sized here, from the
// exact total of this call, before anything is copied -- no gather can outgrow them.
rkh_status gather_goal_probes(rkh_planner* p, std::vector<uint64_t>& gd_off, std::vector<uint64_t>& gd_cnt) {
  gd_off.assign(p->P, 0);
  gd_cnt.assign(p->P, 0);
  uint64_t total = 0;
  for (uint32_t i = 0; i < p->P; ++i) {
    gd_cnt[i] = new_goal_probes(p->prob[i]);
    if (gd_cnt[i]) gd_off[i] = total;
    total += gd_cnt[i];
  }
  if (total > p->h_gd.size()) RKH_TRY(p->h_gd.alloc(total + total / 2 + 1024));
  if (!total) return RKH_OK;
  if (total > p->d_gd.size()) RKH_TRY(p->d_gd.alloc(total + total / 2 + 1024));
  uint32_t n_seg = 0;
  for (uint32_t i = 0; i < p->P; ++i)
    if (gd_cnt[i]) {
      GoalSeg& g = p->h_gd_tab[n_seg++];
      g.src = p->prob[i].d_goal_dist + p->prob[i].goal_checked;
      g.dst_off = gd_off[i];
      g.count = gd_cnt[i];
    }
  RKH_HIP(hipMemcpyAsync(p->d_gd_tab, p->h_gd_tab, n_seg * sizeof(GoalSeg), hipMemcpyHostToDevice, p->stream));
  hipLaunchKernelGGL(gather_goal_dist_kernel, dim3(n_seg), dim3(256), 0, p->stream, p->d_gd_tab, p->d_gd.get());
  RKH_HIP(hipGetLastError());
  RKH_HIP(hipMemcpyAsync(p->h_gd.get(), p->d_gd.get(), total * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  RKH_HIP(hipStreamSynchronize(p->stream));
  return RKH_OK;
}

// edge_added: a finite goal-probe distance registers a solution if it beats the best so far
// (planning_visitors.hpp:194-200, solution_path_factories.hpp:58-110); keep_going() then also checks
// max_num_results (p2p_planning_query.hpp:121-123).  gd[k], k < cnt: the goal-probe result of vertex goal_checked + 1 + k.
rkh_status register_solutions(rkh_planner* p, uint32_t i, const double* gd, uint64_t cnt) {
  Problem& q = p->prob[i];
  const PlannerState& hs = q.h_state;
  const uint64_t first = q.goal_checked;
  std::vector<double> pos;
  std::vector<uint32_t> par;
  for (uint64_t k = 0; k < cnt; ++k) {
    if (!(gd[k] < INFINITY)) continue;
    if (pos.empty()) {
      pos.resize(uint64_t(hs.n) * p->DP);
      par.resize(hs.n);
      RKH_HIP(hipMemcpy(pos.data(), q.d_tree, pos.size() * sizeof(double), hipMemcpyDeviceToHost));
      RKH_HIP(hipMemcpy(par.data(), q.d_parent, par.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    double total = gd[k];
    uint64_t v = first + k + 1;
    while (par[v] != 0xFFFFFFFFu) {
      const uint64_t pv = par[v];
      double acc = 0.0;
      for (int d = 0; d < p->D; ++d) {
        const double df = pos[pv * p->DP + d] - pos[v * p->DP + d];
        acc += df * df;
      }
      total += std::sqrt(acc);
      v = pv;
    }
    if (q.num_solutions == 0 || total < q.best_cost) {
      q.best_cost = total;
      q.best_vertex = uint32_t(first + k + 1);
      ++q.num_solutions;
      if (q.num_solutions >= q.prm.max_results) {
        // the sequential planner stops right after this vertex: drop what speculation added beyond it
        q.truncated = true;
        q.final_n = first + k + 2;
        uint32_t smp = 0;
        RKH_HIP(hipMemcpy(&smp, q.d_node_sample + (first + k + 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
        q.final_iterations = uint64_t(smp) + 1;
        const uint32_t one = 1;  // freeze the problem on the device as well
        RKH_HIP(hipMemcpy(&p->d_states[i].done, &one, sizeof(uint32_t), hipMemcpyHostToDevice));
        break;
      }
    }
  }
  q.goal_checked = first + cnt;
  return RKH_OK;
}

}  // namespace

extern "C" {

rkh_status rkh_planner_create_batch(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prms,
                                    uint32_t n_problems, rkh_planner** out) {
  if (!space) return RKH_ERR_BAD_ARG;
  if (scene && scene->host.planar && !scene->host.planar_dynamics) {
    set_error("this planar (2D) chain was given at position level (no actuators / inertias): quasi-static spaces only");
    return RKH_ERR_UNSUPPORTED;
  }
  return planner_create_common(scene, space, nullptr, prms, n_problems, out);
}

rkh_status rkh_planner_create_qs_batch(rkh_scene* scene, const rkh_qs_space* space, const rkh_rrt_params* prms,
                                       uint32_t n_problems, rkh_planner** out) {
  if (!space) return RKH_ERR_BAD_ARG;
  return planner_create_common(scene, nullptr, space, prms, n_problems, out);
}

rkh_status rkh_planner_create(rkh_scene* scene, const rkh_dyn_space* space, const rkh_rrt_params* prm,
                              rkh_planner** out) {
  return rkh_planner_create_batch(scene, space, prm, 1, out);
}

uint32_t rkh_planner_num_problems(const rkh_planner* p) { return p ? p->P : 0; }

rkh_status rkh_planner_destroy(rkh_planner* p) {
  delete p;  // ~rkh_planner waits for both streams
  return RKH_OK;
}

void* rkh_planner_stream(rkh_planner* p) { return p ? (void*)p->stream : nullptr; }

rkh_status rkh_planner_nn_profile(rkh_planner* p, double* total_ms, uint64_t* total_bytes, uint64_t* launches) {
  if (!p || !total_ms || !total_bytes || !launches) return RKH_ERR_BAD_ARG;
  *total_ms = 0.0;
  *total_bytes = 0;
  *launches = 0;
  if (!p->profile_nn || p->prof_rounds == 0) return RKH_OK;
  RKH_HIP(hipStreamSynchronize(p->stream));
  std::vector<uint64_t> rows(p->prof_rounds, 0);
  std::vector<uint32_t> rn(p->prof_rounds);
  for (Problem& q : p->prob) {
    RKH_HIP(hipMemcpy(rn.data(), q.d_round_n, rn.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < p->prof_rounds; ++r) rows[r] += rn[r];
  }
  for (uint32_t r = 0; r < p->prof_rounds; ++r) {
    if (rows[r] == 0) continue;  // no-op round after completion
    float ms = 0.f;
    RKH_HIP(hipEventElapsedTime(&ms, p->ev[2 * r], p->ev[2 * r + 1]));
    *total_ms += ms;
    *total_bytes += rows[r] * p->DP * sizeof(double);  // algorithmic bytes of one launch: sum over problems of n * D * 8
    *launches += 1;
  }
  return RKH_OK;
}

rkh_status rkh_planner_nn_pairs(rkh_planner* p, uint64_t* pairs) {
  if (!p || !pairs) return RKH_ERR_BAD_ARG;
  *pairs = 0;
  if (!p->profile_nn || p->prof_rounds == 0) return RKH_OK;
  RKH_HIP(hipStreamSynchronize(p->stream));
  std::vector<uint32_t> rn(p->prof_rounds), rb(p->prof_rounds);
  for (Problem& q : p->prob) {
    RKH_HIP(hipMemcpy(rn.data(), q.d_round_n, rn.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    RKH_HIP(hipMemcpy(rb.data(), q.d_round_n + rkh_planner::kProfMax, rb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < p->prof_rounds; ++r) *pairs += uint64_t(rn[r]) * rb[r];
  }
  return RKH_OK;
}

rkh_status rkh_planner_steer_profile(rkh_planner* p, double* total_ms, uint64_t* launches) {
  if (!p || !total_ms || !launches) return RKH_ERR_BAD_ARG;
  *total_ms = 0.0;
  *launches = 0;
  if (!p->profile_nn || p->prof_rounds == 0) return RKH_OK;
  RKH_HIP(hipStreamSynchronize(p->stream));
  for (uint32_t r = 0; r < p->prof_rounds; ++r) {
    float ms = 0.f;
    RKH_HIP(hipEventElapsedTime(&ms, p->ev_steer[2 * r], p->ev_steer[2 * r + 1]));
    *total_ms += ms;
    *launches += 1;
  }
  return RKH_OK;
}

rkh_status rkh_planner_steer_steps(rkh_planner* p, uint64_t* executed_steps) {
  if (!p || !executed_steps) return RKH_ERR_BAD_ARG;
  *executed_steps = 0;
  if (!p->d_steps_exec) return RKH_OK;
  RKH_HIP(hipStreamSynchronize(p->stream));
  unsigned long long v = 0;
  RKH_HIP(hipMemcpy(&v, p->d_steps_exec, sizeof(v), hipMemcpyDeviceToHost));
  *executed_steps = v;
  return RKH_OK;
}

rkh_status rkh_diag_planner_carry_counts(rkh_planner* p, uint64_t counts[2]) {
  if (!p || !counts) return RKH_ERR_BAD_ARG;
  RKH_TRY(read_states(p));
  counts[0] = counts[1] = 0;
  for (const Problem& q : p->prob) {
    counts[0] += q.h_state.cand_discarded;
    counts[1] += q.h_state.cand_reused;
  }
  return RKH_OK;
}

rkh_status rkh_diag_planner_probe_counts(rkh_planner* p, uint32_t problem, uint64_t counts[5], double* reach_q) {
  if (!p || problem >= p->P || !counts) return RKH_ERR_BAD_ARG;
  RKH_TRY(read_states(p));
  const Problem& q = p->prob[problem];
  const PlannerState& hs = q.h_state;
  counts[0] = hs.probes_certified;
  counts[1] = hs.probes_run;
  counts[2] = hs.probed_n;
  counts[3] = hs.list_n;
  uint32_t first = hs.n;  // the first vertex whose probe is open
  if (hs.list_n) RKH_HIP(hipMemcpy(&first, q.d_probe_list, sizeof(uint32_t), hipMemcpyDeviceToHost));
  counts[4] = first;
  if (reach_q) *reach_q = p->reach.reach_q;
  return RKH_OK;
}

rkh_status rkh_diag_planner_sample_cap(rkh_planner* p, uint32_t problem, uint64_t* samples) {
  if (!p || problem >= p->P || !samples) return RKH_ERR_BAD_ARG;
  *samples = p->prob[problem].sample_cap;
  return RKH_OK;
}

rkh_status rkh_planner_enqueue(rkh_planner* p, uint32_t rounds) {
  if (!p) return RKH_ERR_BAD_ARG;
  // make sure the enqueued rounds cannot run out of samples (usually already there: see below)
  const uint64_t share = uint64_t(rounds ? rounds : 1) * p->b_max;
  RKH_TRY(upload_samples_all(p, share, 0));
  for (uint32_t r = 0; r < rounds; ++r) RKH_TRY(enqueue_round(p));
  // while the GPU works on these rounds: the next call's share of the stream (generated on the host, copied behind the
  // rounds on the same stream)
  return rounds ? upload_samples_all(p, 2 * share, 1) : RKH_OK;
}

rkh_status rkh_planner_sync(rkh_planner* p, rkh_planner_stats* stats) {
  if (!p) return RKH_ERR_BAD_ARG;
  RKH_TRY(read_round_results(p));
  std::vector<uint64_t> gd_off, gd_cnt;
  RKH_TRY(gather_goal_probes(p, gd_off, gd_cnt));
  // per problem: grow the sample buffers, register solutions, fill the stats
  for (uint32_t i = 0; i < p->P; ++i) {
    Problem& q = p->prob[i];
    PlannerState& hs = q.h_state;
    if (!q.truncated && hs.done != 1 && uint64_t(hs.s0) + 64ull * p->b_max > q.sample_cap) {
      RKH_HIP(hipStreamSynchronize(p->copy_stream));
      RKH_TRY(grow_sample_buffers(p, i, std::max<uint64_t>(2 * q.sample_cap, uint64_t(hs.s0) + 256ull * p->b_max)));
    }
    if (hs.done == 2 && q.samples_ready < q.sample_cap) {  // sample stream ran dry mid-enqueue: refill and carry on
      hs.done = 0;
      RKH_HIP(hipMemcpy(&p->d_states[i].done, &hs.done, sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (gd_cnt[i]) RKH_TRY(register_solutions(p, i, p->h_gd.get() + gd_off[i], gd_cnt[i]));
    if (stats) {
      rkh_planner_stats& o = stats[i];
      std::memset(&o, 0, sizeof(o));
      o.num_vertices = q.truncated ? q.final_n : hs.n;
      o.iterations = q.truncated ? q.final_iterations : hs.s0;
      o.edges_checked = o.iterations + (o.num_vertices - 1);
      o.edges_speculated = hs.edges_speculated + (hs.n - 1);
      o.rounds = hs.rounds;
      o.num_solutions = q.num_solutions;
      o.best_cost = q.best_cost;
      o.done = (q.truncated || hs.done == 1) ? 1u : 0u;
    }
  }
  return RKH_OK;
}

// The best registered solution as a vertex path root -> ... -> v (the motion then goes on to the goal, which the goal
// probe of v reached): register_basic_solution_path_impl (solution_path_factories.hpp:58-110) walks the same parents.
rkh_status rkh_planner_get_solution(rkh_planner* p, uint32_t problem, uint32_t* path, uint32_t capacity,
                                    uint32_t* n_path, double* cost) {
  if (!p || problem >= p->P || !n_path) return RKH_ERR_BAD_ARG;
  Problem& q = p->prob[problem];
  *n_path = 0;
  if (cost) *cost = q.best_cost;
  if (q.best_vertex == 0xFFFFFFFFu) return RKH_OK;  // no solution registered
  RKH_HIP(hipStreamSynchronize(p->stream));
  std::vector<uint32_t> par(size_t(q.best_vertex) + 1);
  RKH_HIP(hipMemcpy(par.data(), q.d_parent, par.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> rev;
  for (uint32_t v = q.best_vertex; v != 0xFFFFFFFFu; v = par[v]) rev.push_back(v);
  *n_path = uint32_t(rev.size());
  if (path) {
    if (capacity < rev.size()) {
      set_error("rkh_planner_get_solution: path buffer too small");
      return RKH_ERR_CAPACITY;
    }
    for (size_t i = 0; i < rev.size(); ++i) path[i] = rev[rev.size() - 1 - i];
  }
  return RKH_OK;
}

rkh_status rkh_planner_solve(rkh_planner* p, rkh_planner_stats* stats) {
  if (!p) return RKH_ERR_BAD_ARG;
  std::vector<rkh_planner_stats> local(p->P);
  for (;;) {
    rkh_status st = rkh_planner_enqueue(p, 16);
    if (st != RKH_OK) return st;
    st = rkh_planner_sync(p, local.data());
    if (st != RKH_OK) return st;
    bool all = true;
    for (uint32_t i = 0; i < p->P; ++i) {
      if (!local[i].done) all = false;
      Problem& q = p->prob[i];
      if (!local[i].done && q.samples_ready >= q.sample_cap && q.h_state.s0 + p->b_max > q.sample_cap) {
        set_error("planner: sample stream buffers did not grow (out of device memory?)");  // rkh_planner_sync grows them
        return RKH_ERR_CAPACITY;
      }
    }
    if (all) break;
  }
  if (stats) std::memcpy(stats, local.data(), p->P * sizeof(rkh_planner_stats));
  return RKH_OK;
}

rkh_status rkh_planner_get_tree(rkh_planner* p, uint32_t problem, double* pos, uint32_t* parent, uint32_t* nn_seq,
                                uint8_t* accept, double* goal_dist) {
  if (!p || problem >= p->P) return RKH_ERR_BAD_ARG;
  if (goal_dist) RKH_TRY(flush_probes(p));  // make sure no goal probe is pending
  RKH_HIP(hipStreamSynchronize(p->stream));
  Problem& q = p->prob[problem];
  const uint64_t n = q.truncated ? q.final_n : q.h_state.n;
  const uint64_t it = q.truncated ? q.final_iterations : q.h_state.s0;
  if (pos) {
    if (p->DP == p->D) {
      RKH_HIP(hipMemcpy(pos, q.d_tree, n * p->D * sizeof(double), hipMemcpyDeviceToHost));
    } else {
      std::vector<double> tmp(n * p->DP);
      RKH_HIP(hipMemcpy(tmp.data(), q.d_tree, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; ++i) std::memcpy(pos + i * p->D, &tmp[i * p->DP], p->D * sizeof(double));
    }
  }
  if (parent) RKH_HIP(hipMemcpy(parent, q.d_parent, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nn_seq && it) RKH_HIP(hipMemcpy(nn_seq, q.d_nn_seq, it * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (accept && it) RKH_HIP(hipMemcpy(accept, q.d_accept_log, it, hipMemcpyDeviceToHost));
  if (goal_dist && n > 1) RKH_HIP(hipMemcpy(goal_dist, q.d_goal_dist, (n - 1) * sizeof(double), hipMemcpyDeviceToHost));
  return RKH_OK;
}

}  // extern "C"
