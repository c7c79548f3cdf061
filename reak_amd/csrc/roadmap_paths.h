// roadmap_paths.h -- the batched single-source shortest-path search over roadmaps (roadmap_paths.hip) as its callers see
// it: one job per (roadmap, source) pair, a device table of jobs, one launch.
#pragma once
#include "rkh_internal.h"
#include "roadmap_csr.h"

namespace rkh {

constexpr uint32_t kSsspLdsMaxVertices = 4096;  // distances of a roadmap up to this size live in LDS (32 KiB of 160)

// One search.  All pointers are device pointers; the CSR is roadmap_csr.h's (col < n).  The source is the seed list:
// (seed_v[i], seed_d[i]) starts vertex seed_v[i] at distance seed_d[i] >= 0; a roadmap vertex s is the list {(s, 0.0)}.
struct SsspJob {
  const uint32_t* row_ptr = nullptr;  // [n + 1]
  const uint32_t* col = nullptr;      // [row_ptr[n]]
  const double* w = nullptr;          // [row_ptr[n]], >= 0
  uint32_t n = 0;
  uint32_t n_seeds = 0;
  const uint32_t* seed_v = nullptr;
  const double* seed_d = nullptr;
  uint32_t seed_mark = 0xFFFFFFFFu;   // pred of a vertex whose seed is its distance: 0xFFFFFFFF (a roadmap vertex as the
                                      // source) or RKH_PRM_QUERY_POINT
  double* dist = nullptr;             // [n], never null (the global form relaxes in it)
  uint32_t* pred = nullptr;           // [n] or null
  uint32_t* rounds = nullptr;         // relaxation rounds this search ran, or null
};

// The vertex count up to which a launch takes the LDS form: kSsspLdsMaxVertices, lowered by RKH_PRM_PATHS_LDS_MAX.
uint32_t sssp_lds_max();
// n_jobs searches in one launch, one workgroup each; n_max = the largest SsspJob::n among them (chooses the form).
rkh_status launch_roadmap_sssp(hipStream_t s, const SsspJob* d_jobs, uint32_t n_jobs, uint32_t n_max);
// distances from `source` by a single-thread std::priority_queue Dijkstra on the host: what rkh_diag_prm_search_ms times
// the launch against (reference code, not the code under test)
void host_dijkstra(const RoadmapCsr& g, uint32_t source, std::vector<double>* dist);

}  // namespace rkh
