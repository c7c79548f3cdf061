// round_carry.h -- the rule by which a round of the speculative-batch RRT driver (planner.hip) reuses the steered edges
// of the candidates the round before it discarded, stated once.
//
// A round steers B candidates per problem and consumes `cut` of them; candidates [cut, B) are thrown away and the next
// round starts at sample s0 + cut, so its candidate b' is the sample that was candidate b' + cut.  commit_kernel keeps
// the discarded candidates' results (end state, accept bit, step count) and the tree row each was steered from in a stash,
// packed from slot 0.  An edge is a pure function of (source row, sample row): tree rows never change once committed,
// sample rows never change, the scene and the dynamics are constants of the planner.  So where the fresh NN sweep names
// the row the stashed edge was steered from, the stashed results ARE what the steer kernel would write, bit for bit, and
// the steer of that candidate is skipped (carry_restore_kernel, launch 0 of propagate_pair_step_kernel).
//
// The rules use no device builtin and no HIP header, so a host compiler and a sanitizer can read them on a machine
// without a GPU (tests/cpp/round_carry_test.cpp).
#pragma once
#include <cstdint>

#ifndef RKH_HD
#ifdef __HIPCC__
#define RKH_HD __host__ __device__ __forceinline__
#else
#define RKH_HD inline
#endif
#endif

namespace rkh {

// The slot mapping: candidate b_new of the next round was candidate b_new + cut of this one.
RKH_HD uint32_t carry_old_slot(uint32_t b_new, uint32_t cut) { return b_new + cut; }

// Candidates a round of B_old that consumed `cut` leaves in the stash (stash slot j = old slot carry_old_slot(j, cut)).
// valid == false -- the feature is off, the problem is done -- leaves none.
RKH_HD uint32_t carry_count(uint32_t B_old, uint32_t cut, bool valid) { return (valid && cut < B_old) ? B_old - cut : 0u; }

// ... of which a round of B_new candidates can look at: a smaller round drops the surplus (those samples are steered again
// when their turn comes; nothing tries to keep them).
RKH_HD uint32_t carry_usable(uint32_t carried, uint32_t B_new) { return carried < B_new ? carried : B_new; }

// The reuse predicate: slot b_new takes the stashed results iff it is a carried slot and the fresh nearest neighbour is
// the row the stashed edge was steered from.  stash_nn[j] = nn_idx_old[carry_old_slot(j, cut)].
template <class IdxP>
RKH_HD bool carry_reuses(uint32_t b_new, uint32_t carried, uint32_t B_new, uint32_t nn_new, IdxP stash_nn) {
  return b_new < carry_usable(carried, B_new) && nn_new == stash_nn[b_new];
}

// Which rounds carry: the ones that take the step-wise steer launch (its gate: lo <= edges < hi) with at least
// carry_min_edges edges; kCarryOff as carry_min_edges: none.  The restore kernel and launch 0 of the step kernel both
// decide by this function of the same device-side edge count, so they cannot disagree.
constexpr uint32_t kCarryOff = 0xFFFFFFFFu;
RKH_HD bool carry_round(uint32_t edges, uint32_t lo, uint32_t hi, uint32_t carry_min_edges) {
  return carry_min_edges != kCarryOff && edges >= lo && edges < hi && edges >= carry_min_edges;
}

// The share of the usable carried candidates the wave fit expects to be reused, 7/8: the round simulation over the golden
// runs finds 0.84 .. 0.89 of the discarded candidates' nearest neighbours older than the round (tests/
// test_round_carry_cpu.py).  An estimate only: it sizes batches, results do not depend on it.
constexpr uint32_t kCarryReuseNum = 7, kCarryReuseDen = 8;
RKH_HD uint32_t carry_expected_reuse(uint32_t carried, uint32_t B_new) {
  return carry_usable(carried, B_new) * kCarryReuseNum / kCarryReuseDen;
}

}  // namespace rkh
