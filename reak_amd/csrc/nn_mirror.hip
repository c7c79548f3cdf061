// nn_mirror.hip -- the planner-regime 1-NN sweep over the half-precision mirror of the trees (nn_mirror.h).
//
// Replaces min_dist_linear_search (R/ctrl/path_planning/topological_search.hpp:95-118) with euclidean_distance_metric
// (R/ctrl/topologies/vect_distance_metrics.hpp:113-137) for the batches of a planner round: P trees, a few hundred
// queries each, every query against every vertex of its tree.  Exact results (index AND distance, first minimum wins):
// the matrix cores only produce a BOUNDED estimate that selects, per query, the few vertices whose fp64 distance is
// then evaluated with the reference's operation sequence.
//
// Why it is built this way (measured on the kernel it replaces, nn1_sweep_bf16_kernel): that sweep
// was bound by the VALU / LDS work AROUND its matrix instructions -- converting fp64 rows to split-bf16 operands for
// every query block that sweeps them (~15 VALU instructions per wave-slab), three matrix instructions and three LDS
// operand reads per 32 x 32 block of pairs, a per-lane candidate list in LDS -- and it re-read each tree once per 128
// queries (1.7 x the algorithmic bytes).  Here
//   * the operands are stored, not staged: one 16-byte load per lane and slab straight into the A operand (rows), one
//     per lane and query group into the B operands (nn1_mirror_prep_kernel builds those once per round);
//   * ONE instruction per 32 x 32 pairs: with half-precision inputs the error of c against |x - q|^2 - |q_h|^2 is
//     relative to the DISTANCE (below), so a single half-precision product has a narrower band than the split bf16 one;
//   * a wave keeps the B operands of up to kMirG x 32 = 384 queries in registers and runs every slab it loads against
//     all of them: a tree is read once per 384 queries, 32 bytes per vertex;
//   * no candidate bookkeeping in the sweep: PASS 1 only takes minima (8 v_min3_f32 per 16 estimates, branch-free) and
//     leaves min_r c per (row slice, query) in NnArgs::est (plain stores: the first version merged the slices with an
//     ordered-integer atomicMin per lane and spent most of its time there); nn1_mirror_thr_kernel turns the minimum over
//     the slices into the query's threshold; PASS 2 repeats the sweep -- same operands, same instruction, bit-identical
//     estimates -- against that FIXED threshold and appends the rows below it to the query's list;
//     nn1_mirror_resolve_kernel evaluates those exactly;
//   * pass 2 only where a query is OPEN: its estimates are pass 1's, so a slice whose minimum est[slice][q] lies above
//     thr[q] holds no row for q's list (mirror_open, nn_mirror.h).  The thr kernel, which reads every est anyway, writes
//     per (tree, slice) the list of the open queries and its length; a pass-2 block takes its queries from the list of
//     its slice (mirror_open_item) and leaves when the list has no block for it.  On planner trees a query is open in
//     one slice, rarely two: a block's 12 groups become one or two, and pass 2 approaches one read of the mirror.
//     The order of a list influences no result: lists of rows are filled by atomics and the resolve kernel decides by
//     (distance, index).  RKH_NN_MIRROR_OPEN=0 keeps the pass over all queries (the lists are then not built).
//   * where the lists live: in rows of their own behind est (nn1_mirror_query_bytes() grows by 2 bytes per slice and
//     query slot for the entries, 16-bit query numbers, and 16 per slot for the 32 lengths), not in the est rows they
//     would fit into once the thresholds are known.  Reuse in place needs every read of a tree's est to precede every
//     write -- a whole tree's est in one block's registers or LDS, 128 KB at 4096 queries x 32 slices -- and saves 80
//     bytes per query slot of an arena that holds megabytes per tree.  One block per tree builds the lists (ballot,
//     prefix over its four waves, plain stores), so the lengths need no zeroing between rounds and the lists come out
//     in query order.
//
// Error bound.  Everything below is in the mirror's PRESCALED units (nn_mirror.h): x, q stand for p x, p q with the tree's
// power of two p, which brings the coordinate bound into [16, 32) -- exact, so the nearest row and every comparison are
// those of the unscaled problem, and the bound holds alike for a box of side 0.002 and one of side 64.  x_h, q_h =
// half(float(x)), half(float(q)) per coordinate, 0 where that half is below the normal range.  The rounding errors are
// MEASURED, not bounded:
//   dx = max over the rows of a tree of |x - x_h| (kept per tree: mirror_store_row's callers raise it, ordered-integer
//        atomicMax on the float's bits), dq = |q - q_h| of the query, delta = dx + dq >= | |x_h - q_h| - |x - q| |;
//   c_real = |x_h|^2 - 2 x_h.q_h = |x_h - q_h|^2 - |q_h|^2  =>  | c_real + |q_h|^2 - s | <= 2 d delta + delta^2
// with s = |x - q|^2, d = sqrt(s).  The instruction sums <= 16 exact products in float (order and intermediate roundings
// unspecified: 15 roundings of 2^-24 on partial sums below S = X^2 + 2 X |q|, X >= |x_h| for every row; no operand is
// subnormal, and the accumulator never flushes) and the float |x_h|^2 of the mirror carries 12 more: together below
// 2^-19 S.  The three stored pieces of |x_h|^2 add up to it exactly while they are normal halves and leave out less
// than 2^-14 otherwise (kMirrorSplitLoss: every row within 0.35 of the origin has such a piece; S >= 16^2, so the term
// widens eps by an eighth at most and by 0.2 % at the planner's scale): eps = 2^-19 S + 2^-14.  So s_r = c_r + |q_h|^2 + e_r with
// |e_r| <= E(d_r) := 2 d_r delta + delta^2 + eps.  Let m be the row of the smallest estimate and r* the true nearest row
// (any row tying with it included): d_r* <= d_m, hence
//   c_r* = s_r* - |q_h|^2 - e_r* <= s_m - |q_h|^2 + E(d_m) = c_m + e_m + E(d_m) <= c_m + 2 E(d_m),
// and d_m <= delta + sqrt(c_m + |q_h|^2 + 2 delta^2 + eps).  Rows with c <= c_min + band(c_min), band = 2 E(that bound)
// (mirror_threshold, nn_mirror.h: evaluated in double, rounded up) are a superset of the candidates; distances that
// differ in the last bits of their sqrt lie far inside the band, so "first minimum wins" is decided by the exact pass
// among them.  At the planner's scale (12-D, |x| ~ 9, nearest neighbours at d ~ 2, p = 8) delta ~ 3e-3 and the band
// ~ 0.03 in squared-distance units of the unscaled problem.  tests/test_nn_mirror_band_cpu.py checks the superset claim
// on a model of the operands.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "nn_device.h"
#include "nn_mirror.h"
#include "rkh_internal.h"
#include "staged_call.h"

namespace rkh {

void nn_set_last_kernel_name(const char* name);  // nn_sweep.hip (rkh_nn_kernel_name)

namespace {

typedef float mir_f16v __attribute__((ext_vector_type(16)));
typedef _Float16 mir_h8 __attribute__((ext_vector_type(8)));

constexpr int kMirG = int(kMirrorGroups);     // query groups of 32 per block
constexpr int kMirQueries = int(kMirrorQueries);  // 384
constexpr int kMirThreads = 256;           // four waves: the same queries, every fourth slab of the block's slice each
constexpr uint32_t kMirCandCap = 32;       // candidate rows kept per query (more: the exact scan of the resolve kernel)
constexpr uint32_t kMirMaxSlices = 32;     // row slices per tree (rows of NnArgs::est)

__device__ __forceinline__ float fmin3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }

// ---- once per round and query: the B operand and the query's share of the error bound
// qinfo[q] = {|q_h|^2 (rounded up), dq = |q - q_h| (rounded up), |q| (rounded up)} of the query times `scale`
__global__ __launch_bounds__(256) void nn1_mirror_prep_kernel(const NnArgs* __restrict__ table, int D, double scale) {
  const NnArgs a = table[blockIdx.y];
  const uint32_t B = a.d_B ? *a.d_B : a.B;
  const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
  if (qi >= B) return;
  const double* __restrict__ qq = a.q + ((a.d_qoff ? uint64_t(*a.d_qoff) : 0ull) + qi) * D;
  uint32_t e[16];
  double qn2 = 0.0, qh2 = 0.0, dq2 = 0.0;
#pragma unroll
  for (int d = 0; d < kMirrorMaxDims; ++d) {
    const double qv = (d < D ? qq[d < D ? d : 0] : 0.0) * scale;  // (scaled after the select: the loads stay independent)
    const uint32_t hb = mirror_operand_bits(float(qv));
    const double qh = double(mirror_half_value(hb));
    qn2 += qv * qv;
    qh2 += qh * qh;
    dq2 += (qv - qh) * (qv - qh);
    e[d] = mirror_half_bits(-2.0f * mirror_half_value(hb));  // exact: a power-of-two multiple of a half
  }
  e[12] = e[13] = e[14] = 0x3C00u;  // 1.0 against the three pieces of |x_h|^2
  e[15] = 0u;
  uint4* __restrict__ qf = a.qfrag + uint64_t(qi) * 2;
  qf[0] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  qf[1] = make_uint4(e[8] | (e[9] << 16), e[10] | (e[11] << 16), e[12] | (e[13] << 16), e[14] | (e[15] << 16));
  double* __restrict__ qi3 = a.qinfo + uint64_t(qi) * 3;
  qi3[0] = qh2 * (1.0 + 1e-12) + 1e-300;
  qi3[1] = sqrt(dq2) * (1.0 + 1e-12);
  qi3[2] = sqrt(qn2) * (1.0 + 1e-12);
}

// ---- between the passes: threshold of a query = (minimum over the row slices) + band; with open_lists, the list of the
// open queries of every slice (NnArgs::open_list, open_cnt).  x_norm_bound is in the mirror's prescaled units.  Lists: grid (1, trees), the block walks its tree's queries
// 256 at a time and appends each slice's open ones in query order -- ballot per wave, prefix over the four waves in
// LDS, plain stores, so nothing needs to be zero when the kernel starts.  Without: grid (ceil(B / 256), trees).
__global__ __launch_bounds__(256) void nn1_mirror_thr_kernel(const NnArgs* __restrict__ table, uint32_t gx,
                                                             double x_norm_bound, uint32_t open_lists) {
  __shared__ uint32_t s_cnt[4][kMirMaxSlices];  // open queries of the current 256 per (wave, slice)
  __shared__ uint32_t s_len[kMirMaxSlices];     // list lengths so far (entry sl is thread sl's alone)
  const NnArgs a = table[blockIdx.y];
  const uint32_t B = a.d_B ? *a.d_B : a.B;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < kMirMaxSlices) s_len[tid] = 0u;
  for (uint32_t qb = blockIdx.x * 256u; qb < B; qb += gridDim.x * 256u) {  // (B is uniform: whole blocks iterate)
    const uint32_t qi = qb + tid;
    const bool live = qi < B;
    float thr = -INFINITY;
    float est[kMirMaxSlices];  // the query's minima, read once (slices past gx: +inf, open nowhere but in an empty tree's
                               // lists, which the loops below do not visit)
#pragma unroll
    for (uint32_t sl = 0; sl < kMirMaxSlices; ++sl)
      est[sl] = (live && sl < gx) ? a.est[uint64_t(sl) * a.est_stride + qi] : INFINITY;
    if (live) {
      float cmin = INFINITY;
#pragma unroll
      for (uint32_t sl = 0; sl < kMirMaxSlices; ++sl) cmin = __builtin_fminf(cmin, est[sl]);
      const double* __restrict__ qi3 = a.qinfo + uint64_t(qi) * 3;
      const double qh2 = qi3[0], dq = qi3[1], qn = qi3[2];
      const double dx = double(__uint_as_float(*a.dx_max_bits));
      // (+inf, an empty tree, stays +inf: every row is a candidate and the resolve kernel sorts it out)
      thr = cmin < INFINITY ? __double2float_ru(mirror_threshold(double(cmin), qh2, dq, qn, dx, x_norm_bound)) : INFINITY;
      a.thr[qi] = thr;
    }
    if (!open_lists) continue;
    // the slices the query is open in, one bit each; a query slot past the batch is never open
    uint32_t open_mask = 0u;
#pragma unroll
    for (uint32_t sl = 0; sl < kMirMaxSlices; ++sl) open_mask |= (live && mirror_open(est[sl], thr)) ? (1u << sl) : 0u;
    for (uint32_t sl = 0; sl < gx; ++sl) {
      const unsigned long long m = __ballot(((open_mask >> sl) & 1u) != 0u);
      if (lane == 0) s_cnt[wave][sl] = uint32_t(__builtin_popcountll(m));
    }
    __syncthreads();
    for (uint32_t sl = 0; sl < gx; ++sl) {
      const bool o = ((open_mask >> sl) & 1u) != 0u;
      const unsigned long long m = __ballot(o);
      uint32_t pos = s_len[sl] + uint32_t(__builtin_popcountll(m & ((1ull << lane) - 1ull)));
      for (uint32_t w = 0; w < wave; ++w) pos += s_cnt[w][sl];
      if (o) a.open_list[uint64_t(sl) * a.est_stride + pos] = uint16_t(qi);  // pos < B: at most one entry per query
    }
    __syncthreads();
    if (tid < gx) s_len[tid] += s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
    __syncthreads();
  }
  if (open_lists && tid < gx) a.open_cnt[tid] = s_len[tid];  // (also for a tree without queries: no stale list is read)
}

// PASS 1: minimum of the estimates per (slice, query) -> NnArgs::est.  PASS 2: rows at or below NnArgs::thr -> lists.
// Work items as in the bf16 sweep (nn_xcd_item), always with a query-block prefix.  PASS 2 with open_lists: item (bx, by)
// is block by of the open list of slice bx (mirror_open_item); the grid is still the host's bound of one block per 384
// queries of the batch and slice, a block past its slice's list leaves.
template <int PASS>
__global__ __launch_bounds__(kMirThreads, PASS == 1 ? 4 : 3) void nn1_mirror_kernel(const NnArgs* __restrict__ table,
                                                                    const uint32_t* __restrict__ yblock_base,
                                                                    uint32_t n_problems, uint32_t gx,
                                                                    uint32_t open_lists) {
  __shared__ float wave_min[PASS == 1 ? kMirThreads / 64 : 1][PASS == 1 ? kMirQueries : 1];
  uint32_t bx, by, bz;
  __builtin_assume(yblock_base != nullptr);
  if (!nn_xcd_item(yblock_base, n_problems, gx, 0u, bx, by, bz)) return;
  const NnArgs a = table[bz];
  const uint4* __restrict__ mirror = static_cast<const uint4*>(nn_uniform(a.mirror));
  const uint4* __restrict__ qfrag = nn_uniform(a.qfrag);
  const uint32_t n = nn_uniform(a.d_n ? *a.d_n : uint32_t(a.n));
  const uint32_t B = nn_queries(a);
  // the block's queries: entries [q0, q0 + it.count) of the batch, or of the open list of its slice (uniform)
  const uint16_t* __restrict__ olist = nullptr;
  uint32_t listed = B;
  if (PASS == 2 && open_lists) {
    olist = nn_uniform(a.open_list) + uint64_t(bx) * a.est_stride;
    listed = nn_uniform(a.open_cnt[bx]);
  }
  const MirrorOpenItem it = mirror_open_item(listed, by);
  if (it.count == 0u) return;
  const uint32_t q0 = it.first;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hi = lane >> 5;
  const int ng = int(it.groups);  // uniform
  const uint32_t qcol = q0 + uint32_t(col);  // the lane's entry of group 0

  // B operands: lane (col, hi) holds slots 8 hi .. 8 hi + 7 of query q0 + 32 g + col
  uint4 bop[kMirG];
  float thr[kMirG];  // PASS 1: running minimum; PASS 2: the fixed threshold
#pragma unroll
  for (int g = 0; g < kMirG; ++g) {
    bop[g] = make_uint4(0u, 0u, 0u, 0u);
    thr[g] = PASS == 1 ? INFINITY : -INFINITY;
    if (g < ng) {
      const uint32_t slot = 32u * uint32_t(g) + uint32_t(col);
      const uint32_t e = mirror_open_entry(it, slot);
      const uint32_t qsrc = (PASS == 2 && olist) ? uint32_t(olist[e]) : e;
      bop[g] = qfrag[uint64_t(qsrc) * 2 + uint32_t(hi)];
      if (PASS == 2) thr[g] = mirror_open_slot_live(it, slot) ? a.thr[qsrc] : -INFINITY;  // a pad slot never records
    }
  }

  // this wave's slabs: every fourth one of the block's contiguous slice of the tree
  const uint32_t slabs_total = (n + 31u) >> 5;
  const uint32_t per_block = (slabs_total + gx - 1u) / gx;
  const uint32_t s_first = bx * per_block;
  uint32_t s_end = s_first + per_block;
  if (s_end > slabs_total) s_end = slabs_total;
  const uint4* __restrict__ my = mirror + uint32_t(lane);
  constexpr uint32_t kStep = 4;
  auto load = [&](uint32_t s) -> uint4 { return my[uint64_t(s < s_end ? s : s_first) * 64u]; };
  uint32_t s = s_first + uint32_t(wave);
  uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0, a2 = a0;
  if (s_first < s_end) {
    a0 = load(s);
    a1 = load(s + kStep);
    a2 = load(s + 2 * kStep);
  }
  mir_f16v zero;
#pragma unroll
  for (int k = 0; k < 16; ++k) zero[k] = 0.0f;
  // one 32 x 32 block of estimates: minimum tree (PASS 1) / threshold test (PASS 2)
  auto settle = [&](int g, const mir_f16v& c, uint32_t slab) {
    const float t1 = fmin3(c[0], c[1], c[2]), t2 = fmin3(c[3], c[4], c[5]), t3 = fmin3(c[6], c[7], c[8]);
    const float t4 = fmin3(c[9], c[10], c[11]), t5 = fmin3(c[12], c[13], c[14]);
    const float t6 = fmin3(t1, t2, t3), t7 = fmin3(t4, t5, c[15]);
    if (PASS == 1) {
      thr[g] = fmin3(t6, t7, thr[g]);
    } else {
      const float m = __builtin_fminf(t6, t7);
      // rare (a few rows per query over the whole tree): a wave-uniform test first, so that the common case falls
      // through one untaken scalar branch (a per-lane `if` compiles to a TAKEN exec-mask branch around the inlined
      // slow path in every block: pass 2 then ran at 0.4 of pass 1's speed)
      if (__builtin_expect(__any(m <= thr[g]), 0) && m <= thr[g]) {
        // the real query, read again from the list.  (The empty asm keeps this path's address arithmetic inside it:
        // hoisted out of the slab loop it holds two registers per group through the sweep, and the kernel spills.)
        uint32_t e = qcol;
        asm volatile("" : "+v"(e));
        e += 32u * uint32_t(g);
        const uint32_t qi = olist ? uint32_t(olist[e]) : e;
        const uint32_t row0 = slab * 32u + 4u * uint32_t(hi);
        uint32_t mask = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) mask |= (c[i] <= thr[g]) ? (1u << i) : 0u;
        const uint32_t cnt = uint32_t(__builtin_popcount(mask));
        uint32_t pos = atomicAdd(&a.cand_cnt[qi], cnt);
#pragma unroll 1
        while (mask) {
          const uint32_t i = uint32_t(__builtin_ctz(mask));
          mask &= mask - 1u;
          const uint32_t row = row0 + 8u * (i >> 2) + (i & 3u);
          if (pos < kMirCandCap) a.cand_rows[uint64_t(qi) * kMirCandCap + pos] = row;
          ++pos;
        }
      }
    }
  };
  // Query groups go in pairs with two accumulators, software-pipelined: the matrix instruction of the next group is
  // issued before the minimum tree of the current one, so a wave's own VALU work covers its matrix latency (one
  // accumulator: 12 wait states behind every instruction, 71 cycles per block at four waves per SIMD).  An odd group
  // count runs one idle group (B operand zero: its estimates are |x_h|^2, its threshold never matches).
  const int npairs = (ng + 1) >> 1;  // uniform
  // (the pair count is a compile-time constant of the loop body: with a run-time bound the conditional re-assignment of
  // the rolling accumulator costs sixteen register copies per pair)
  auto sweep = [&](auto np_c) {
    constexpr int NP = decltype(np_c)::value;
#pragma unroll 1
    for (; s < s_end; s += kStep) {
      const uint4 an = load(s + 3 * kStep);
      const mir_h8 av = __builtin_bit_cast(mir_h8, a0);
      // rolling: the matrix instruction of group g + 1 is in flight while the VALU settles group g
      mir_f16v cA = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(mir_h8, bop[0]), zero, 0, 0, 0);
#pragma unroll
      for (int pr = 0; pr < NP; ++pr) {
        const mir_f16v cB =
            __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(mir_h8, bop[2 * pr + 1]), zero, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler would sink the instruction behind the settling it overlaps)
        settle(2 * pr, cA, s);
        __builtin_amdgcn_sched_barrier(0);
        if (pr + 1 < NP)
          cA = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, __builtin_bit_cast(mir_h8, bop[2 * pr + 2 < kMirG ? 2 * pr + 2 : 0]),
                                                      zero, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        settle(2 * pr + 1, cB, s);
        __builtin_amdgcn_sched_barrier(0);
      }
      a0 = a1;
      a1 = a2;
      a2 = an;
    }
  };
  switch (npairs) {
    case 1: sweep(std::integral_constant<int, 1>()); break;
    case 2: sweep(std::integral_constant<int, 2>()); break;
    case 3: sweep(std::integral_constant<int, 3>()); break;
    case 4: sweep(std::integral_constant<int, 4>()); break;
    case 5: sweep(std::integral_constant<int, 5>()); break;
    default: sweep(std::integral_constant<int, 6>()); break;
  }
  if (PASS == 1) {
    // the block's four waves hold different slabs of the same queries: merge through LDS, one store per query
#pragma unroll
    for (int g = 0; g < kMirG; ++g) {
      if (g < ng) {
        float m = thr[g];
        m = __builtin_fminf(m, __shfl_xor(m, 32, 64));  // the two lane halves hold different rows of the same query
        if (hi == 0) wave_min[wave][32 * g + col] = m;
      }
    }
    __syncthreads();
    for (uint32_t t = uint32_t(tid); t < uint32_t(32 * ng); t += uint32_t(kMirThreads)) {
      const float m = __builtin_fminf(__builtin_fminf(wave_min[0][t], wave_min[1][t]),
                                      __builtin_fminf(wave_min[2][t], wave_min[3][t]));
      if (q0 + t < B) a.est[uint64_t(bx) * a.est_stride + q0 + t] = m;
    }
  }
}

// Exact evaluation of the candidates: one 16-lane group per query, lane j takes the candidates j, j + 16, ...; a list
// that overflowed (more than kMirCandCap rows within the band: many coincident vertices) is replaced by the exact scan
// of the whole tree.  Pad rows (past the end of the tree; a removed vertex evaluates to +inf by itself) are skipped.
// The operation sequence is every sweep's (nn_exact_sq): left-to-right sum of squares, sqrt, lexicographic (distance, index).
template <int DP>
__global__ __launch_bounds__(256) void nn1_mirror_resolve_kernel(const NnArgs* __restrict__ table, int D) {
  const NnArgs a = table[blockIdx.y];
  const uint32_t B = a.d_B ? *a.d_B : a.B;
  const uint32_t qi = blockIdx.x * 16u + (threadIdx.x >> 4);
  const uint32_t gl = threadIdx.x & 15u;
  if (qi >= B) return;  // whole 16-lane groups leave together
  const uint32_t n = a.d_n ? *a.d_n : uint32_t(a.n);
  const double* __restrict__ qq = a.q + ((a.d_qoff ? uint64_t(*a.d_qoff) : 0ull) + qi) * D;
  double qv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = d < D ? qq[d < D ? d : 0] : 0.0;
  const uint32_t cnt = a.cand_cnt[qi];
  double bd = INFINITY;
  uint32_t bi = 0xFFFFFFFFu;
  auto exact = [&](uint32_t row) {
    if (row >= n) return;
    const double* __restrict__ p = a.pos + uint64_t(row) * DP;
    const double dd = sqrt(nn_exact_sq<DP>([&](int d) { return qv[d] - p[d]; }));
    if (lex_less(dd, row, bd, bi)) {
      bd = dd;
      bi = row;
    }
  };
  if (cnt <= kMirCandCap) {
    for (uint32_t j = gl; j < cnt; j += 16u) exact(a.cand_rows[uint64_t(qi) * kMirCandCap + j]);
  } else {
    for (uint32_t row = gl; row < n; row += 16u) exact(row);
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const double od = __shfl_xor(bd, off, 64);
    const uint32_t oi = __shfl_xor(bi, off, 64);
    if (lex_less(od, oi, bd, bi)) {
      bd = od;
      bi = oi;
    }
  }
  if (gl == 0) {
    a.idx[qi] = bi;
    a.dist[qi] = bd;
    a.cand_cnt[qi] = 0u;  // consumed: ready for the next round
  }
}

__global__ __launch_bounds__(256) void mirror_fill_kernel(uint4* __restrict__ mirror, uint64_t slabs) {
  const uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;  // one 16-byte fragment each
  if (i >= slabs * 64u) return;
  mirror[i] = mirror_pad_fragment(i);
}

__global__ __launch_bounds__(256) void mirror_build_kernel(uint4* __restrict__ mirror, const double* __restrict__ pos,
                                                           uint64_t n, int D, int DP, double scale,
                                                           uint32_t* __restrict__ dx_max_bits) {
  const uint64_t row = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (row >= n) return;
  mirror_store_row(mirror, row, pos + row * DP, D, scale, dx_max_bits);
}

}  // namespace

uint32_t nn1_mirror_queries() { return uint32_t(kMirQueries); }
uint32_t nn1_mirror_cand_cap() { return kMirCandCap; }
uint32_t nn1_mirror_max_slices() { return kMirMaxSlices; }
size_t nn1_mirror_bytes(uint64_t capacity_rows) { return size_t((capacity_rows + 31) / 32) * 1024; }
// per-query scratch of a tree's sweeps, in bytes per query slot: B operand (32) + qinfo (24) + threshold (4) +
// candidate count (4) + candidate rows + the per-slice minima + the per-slice open lists (16-bit entries) + 16 for the
// lists' lengths (4 * kMirMaxSlices bytes per tree, and b_max >= 8)
static_assert(kMirMaxSlices * sizeof(uint32_t) <= 8 * 16, "the open lists' lengths take 16 bytes of 8 query slots");
size_t nn1_mirror_query_bytes() {
  return 32 + 24 + 4 + 4 + 4 * size_t(kMirCandCap) + 4 * size_t(kMirMaxSlices) + 2 * size_t(kMirMaxSlices) + 16;
}
// carve a block of nn1_mirror_query_bytes() * b_max bytes (b_max a multiple of 8, base 256-byte aligned) into the
// per-query arrays of `a`
void nn1_mirror_carve(void* base, uint32_t b_max, NnArgs* a) {
  char* p = static_cast<char*>(base);
  a->qfrag = reinterpret_cast<uint4*>(p);
  p += size_t(b_max) * 32;
  a->qinfo = reinterpret_cast<double*>(p);
  p += size_t(b_max) * 24;
  a->thr = reinterpret_cast<float*>(p);
  p += size_t(b_max) * 4;
  a->cand_cnt = reinterpret_cast<uint32_t*>(p);
  p += size_t(b_max) * 4;
  a->cand_rows = reinterpret_cast<uint32_t*>(p);
  p += size_t(b_max) * 4 * kMirCandCap;
  a->est = reinterpret_cast<float*>(p);
  a->est_stride = b_max;
  p += size_t(b_max) * 4 * kMirMaxSlices;
  a->open_list = reinterpret_cast<uint16_t*>(p);  // rows of est_stride entries, like est
  p += size_t(b_max) * 2 * kMirMaxSlices;
  a->open_cnt = reinterpret_cast<uint32_t*>(p);
}

// RKH_NN_MIRROR_OPEN=0: pass 2 over all queries of the batch, as before the open lists (results are the same).  A
// planner reads the switch once, when it is created (tune_planner).  rkh_diag_nn_mirror_query has no handle to keep
// it in and reads it again at every call, on purpose: tests/test_nn_mirror_open_gpu.py compares the two forms in one
// process.
bool nn1_mirror_open_lists() {
  const char* e = getenv("RKH_NN_MIRROR_OPEN");
  return !e || atoi(e) != 0;
}

// does the mirror sweep take this problem shape?
bool nn1_mirror_applies(int D, double coord_bound) {
  return D >= 1 && D <= kMirrorMaxDims && coord_bound >= kMirrorMinBound && coord_bound <= kMirrorMaxBound;
}

rkh_status launch_mirror_fill(hipStream_t s, void* d_mirror, uint64_t capacity_rows) {
  const uint64_t slabs = (capacity_rows + 31) / 32;
  hipLaunchKernelGGL(mirror_fill_kernel, dim3(uint32_t((slabs * 64 + 255) / 256)), dim3(256), 0, s,
                     static_cast<uint4*>(d_mirror), slabs);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

rkh_status launch_mirror_build(hipStream_t s, void* d_mirror, const double* d_pos, uint64_t n, int D, int DP, double scale,
                               uint32_t* d_dx_max_bits) {
  if (n == 0) return RKH_OK;
  hipLaunchKernelGGL(mirror_build_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, s, static_cast<uint4*>(d_mirror),
                     d_pos, n, D, DP, scale, d_dx_max_bits);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// The launches of a round's NN search over the mirrors: B operands, pass 1, thresholds, pass 2, exact resolution.
// d_yblock_base: [n_problems + 1] exclusive prefix of ceil(B_p / nn1_mirror_queries()); n_upper / B_upper (host bounds)
// only size the grids; x_norm_bound >= |x| for every vertex; scale = the mirrors' prescale (mirror_prescale of the
// coordinate bound they were written with).  ev0 / ev1 bracket all five launches.
rkh_status launch_nn1_mirror(hipStream_t s, int D, const NnArgs* d_table, uint32_t n_problems, uint64_t n_upper,
                             uint32_t B_upper, double x_norm_bound, double scale, const uint32_t* d_yblock_base,
                             bool open_lists, hipEvent_t ev0, hipEvent_t ev1) {
  if (B_upper == 0 || n_problems == 0) return RKH_OK;
  if (B_upper > 0xFFFFu) open_lists = false;  // (list entries are 16-bit query numbers; a planner's batch is <= 4096)
  const uint32_t gy = (B_upper + kMirQueries - 1) / kMirQueries;
  const uint64_t slabs = (n_upper + 31) / 32;
  // row slices per tree: ~8 k blocks over the whole grid, at least 32 slabs (8 per wave) per block
  uint64_t gx = 8192 / (uint64_t(gy) * n_problems);
  if (gx > slabs / 32) gx = slabs / 32;
  if (gx > kMirMaxSlices) gx = kMirMaxSlices;
  if (gx < 1) gx = 1;
  const dim3 grid(uint32_t((gx * gy * n_problems + 7) / 8 * 8));
  const dim3 qgrid((B_upper + 255) / 256, n_problems);
  nn_set_last_kernel_name("nn1_mirror_kernel");
  if (ev0) (void)hipEventRecord(ev0, s);
  hipLaunchKernelGGL(nn1_mirror_prep_kernel, qgrid, dim3(256), 0, s, d_table, D, scale);
  hipLaunchKernelGGL((nn1_mirror_kernel<1>), grid, dim3(kMirThreads), 0, s, d_table, d_yblock_base, n_problems, uint32_t(gx),
                     0u);
  hipLaunchKernelGGL(nn1_mirror_thr_kernel, open_lists ? dim3(1, n_problems) : qgrid, dim3(256), 0, s, d_table, uint32_t(gx),
                     x_norm_bound * scale, open_lists ? 1u : 0u);
  hipLaunchKernelGGL((nn1_mirror_kernel<2>), grid, dim3(kMirThreads), 0, s, d_table, d_yblock_base, n_problems, uint32_t(gx),
                     open_lists ? 1u : 0u);
  const dim3 rgrid((B_upper + 15) / 16, n_problems);
  bool resolved = false;  // (the resolve kernel exists for the widths a mirror fragment holds)
  with_padded_dims(D, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if constexpr (DP <= kMirrorMaxDims) {
      hipLaunchKernelGGL((nn1_mirror_resolve_kernel<DP>), rgrid, dim3(256), 0, s, d_table, D);
      resolved = true;
    }
  });
  if (!resolved) {
    set_error("nn mirror: unsupported dimension");
    return RKH_ERR_BAD_ARG;
  }
  if (ev1) (void)hipEventRecord(ev1, s);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

}  // namespace rkh

// Diagnostics (include/rkh_diag.h): the mirror sweep on a caller's point cloud, outside a planner -- the parity tests
// drive it with adversarial clouds (duplicates, one-ulp neighbours, more coincident vertices than a candidate list holds).
extern "C" rkh_status rkh_diag_nn_mirror_query(rkh_ctx* ctx, const double* pts, uint64_t n, int D, const double* q,
                                               uint32_t B, double coord_bound, uint32_t* idx, double* dist) {
  using namespace rkh;
  if (!ctx || !pts || !q || !idx || !dist || n == 0 || B == 0) return RKH_ERR_BAD_ARG;
  if (!nn1_mirror_applies(D, coord_bound)) {
    set_error("nn mirror: needs 1 <= D <= 12 and a coordinate bound in [1e-3, 32]");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int DP = nn_padded_dims(D);
  std::vector<double> rows(size_t(n) * DP, 0.0);
  for (uint64_t i = 0; i < n; ++i)
    for (int d = 0; d < D; ++d) rows[i * DP + d] = pts[i * D + d];
  const uint32_t Bp = (B + 7u) / 8u * 8u;
  const uint32_t yb[2] = {0u, (B + nn1_mirror_queries() - 1) / nn1_mirror_queries()};
  NnArgs a;  // filled below; like rows and yb declared before the call that uploads it
  StagedCall call(s);
  a.pos = call.in(rows.data(), rows.size());
  a.n = n;
  a.q = call.in(q, size_t(B) * D);
  a.B = B;
  a.idx = call.out(idx, B);
  a.dist = call.out(dist, B);
  void* d_scratch = call.scratch<char>(nn1_mirror_query_bytes() * Bp, 0, 0);
  const uint32_t* d_yb = call.in(yb, 2);
  uint32_t* d_dx = call.scratch<uint32_t>(1, 0, 0);
  void* d_mirror = call.scratch<char>(nn1_mirror_bytes(n));
  RKH_TRY(call.status());
  a.dx_max_bits = d_dx;
  a.mirror = d_mirror;
  nn1_mirror_carve(d_scratch, Bp, &a);
  const NnArgs* d_tab = call.in(&a, 1);
  RKH_TRY(call.status());
  RKH_TRY(launch_mirror_fill(s, d_mirror, n));
  const double scale = mirror_prescale(coord_bound);
  RKH_TRY(launch_mirror_build(s, d_mirror, a.pos, n, D, DP, scale, d_dx));
  RKH_TRY(launch_nn1_mirror(s, D, d_tab, 1, n, B, std::sqrt(double(D)) * coord_bound, scale, d_yb, nn1_mirror_open_lists(), nullptr,
                            nullptr));
  return call.fetch();
}
