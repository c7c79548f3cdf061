// roadmap_paths.hip -- batched single-source shortest paths over roadmaps: what prm_planner_visitor::publish_path
// (ctrl/path_planning/prm_path_planner.tpp:97-122) asks of the motion graph -- distance_accum and predecessor of every
// vertex -- for many (roadmap, source) pairs in one launch.  A module of its own: a kernel added to an existing module
// moves the code of the ones it holds.
//
// One workgroup of 256 threads per pair -- 32 groups of 8 lanes, a group per vertex: its lanes read the vertex's CSR row
// side by side and reduce their minima with lane shuffles, which changes no result (the minimum of the same set of sums).
// Nothing is shared between workgroups: no grid-wide barrier, no spinning on memory, no cooperative launch.  The search is
// the pull form of Bellman-Ford: every round each vertex v takes
//     min(dist[v], min over its edges (u, w) of dist[u] + w)          strict <, plain fp64 + (-ffp-contract=off)
// where dist starts from the seed list (+inf elsewhere), so dist[v] <= seed[v] throughout.  Lane 0 of a vertex's group
// writes that vertex's slot and no other; there are no read-modify-write atomics.  Distances only fall, fp64 addition is
// monotone and every weight is
// >= 0 (a + w >= a), so the least fixed point is unique: the minimum over paths of the left-to-right sums from the source,
// which is what a sequential Dijkstra computes, bit for bit, whatever the schedule.  That is why the rounds update in
// place: a round may read a neighbour's value of this round or of the last one, either is an upper bound that only
// delays.  Every read and write of a distance is ONE aligned 8-byte access (sssp_load / sssp_store: a relaxed load / store
// of the double, ds_read_b64 / global_load_dwordx2 and their stores), so no torn value is ever seen.
// Loop bounds: a round that changes no distance ends the search (block-wide OR through LDS); Bellman-Ford needs at most
// n - 1 rounds, the loop is capped at n; every inner loop runs over a CSR row or the seed list.
// Predecessors are one pass after convergence, so they do not depend on the schedule: the lowest u among v's edges with
// dist[u] + w == dist[v]; a vertex whose seed is its distance gets the job's seed_mark; unreached vertices 0xFFFFFFFF.
//
// Storage: the distance row lives in LDS up to sssp_lds_max() vertices (kSsspLdsMaxVertices = 4096: 32 KiB, five
// workgroups per CU), else in the job's global row (the waves of a workgroup share their CU's vector cache and the
// barrier between rounds orders the accesses at workgroup scope).  Same text, same results.
#include <hip/hip_runtime.h>

#include <queue>

#include "roadmap_csr.h"
#include "roadmap_paths.h"
#include "staged_call.h"

namespace rkh {

namespace {
constexpr int kSsspThreads = 256;
constexpr int kSsspGroupLanes = 8;  // lanes that share a vertex: they read its CSR row side by side (coalesced) and reduce
constexpr int kSsspGroups = kSsspThreads / kSsspGroupLanes;

__device__ __forceinline__ double sssp_load(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void sssp_store(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
}  // namespace

template <bool kLds>
__global__ __launch_bounds__(kSsspThreads) void roadmap_sssp_kernel(const SsspJob* __restrict__ jobs, uint32_t n_jobs) {
  __shared__ double s_dist[kLds ? kSsspLdsMaxVertices : 1];
  __shared__ uint32_t s_changed[3];
  const uint32_t job = blockIdx.z * gridDim.y + blockIdx.y;
  if (job >= n_jobs) return;  // (block-uniform)
  const SsspJob j = jobs[job];
  const uint32_t n = j.n, tid = threadIdx.x;
  const uint32_t grp = tid / kSsspGroupLanes, gl = tid % kSsspGroupLanes;  // vertex group of the block, lane of the group
  double* const d = kLds ? s_dist : j.dist;
  for (uint32_t v = tid; v < n; v += kSsspThreads) sssp_store(d + v, INFINITY);
  if (tid < 3) s_changed[tid] = 0u;
  __syncthreads();
  if (tid == 0)  // the seed list is short (one entry, or the accepted connections of a query point)
    for (uint32_t i = 0; i < j.n_seeds; ++i) {
      const uint32_t v = j.seed_v[i];
      const double sd = j.seed_d[i];
      if (sd < sssp_load(d + v)) sssp_store(d + v, sd);
    }
  __syncthreads();
  uint32_t rounds = 0;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t slot = r % 3u;
    if (tid == 0) s_changed[(r + 1u) % 3u] = 0u;  // read last in round r - 2, written next in round r + 1
    bool changed = false;
    for (uint32_t v = grp; v < n; v += kSsspGroups) {  // (uniform over the lanes of a group)
      const double old = sssp_load(d + v);
      double best = old;
      const uint32_t e1 = j.row_ptr[v + 1];
      for (uint32_t e = j.row_ptr[v] + gl; e < e1; e += kSsspGroupLanes) {
        const double c = sssp_load(d + j.col[e]) + j.w[e];
        if (c < best) best = c;
      }
#pragma unroll
      for (int m = kSsspGroupLanes / 2; m > 0; m >>= 1) {  // the minimum over the group's lanes: the same set of sums
        const double o = __shfl_xor(best, m, kSsspGroupLanes);
        if (o < best) best = o;
      }
      if (gl == 0 && best < old) {
        sssp_store(d + v, best);
        changed = true;
      }
    }
    if (changed) s_changed[slot] = 1u;
    __syncthreads();
    ++rounds;
    if (s_changed[slot] == 0u) break;  // (block-uniform)
  }
  // predecessors, from the converged distances alone
  for (uint32_t v = grp; v < n; v += kSsspGroups) {
    const double dv = sssp_load(d + v);
    if (kLds && gl == 0) j.dist[v] = dv;
    if (!j.pred) continue;  // (block-uniform)
    uint32_t best = 0xFFFFFFFFu;
    if (dv != INFINITY) {
      const uint32_t e1 = j.row_ptr[v + 1];
      for (uint32_t e = j.row_ptr[v] + gl; e < e1; e += kSsspGroupLanes) {
        const uint32_t u = j.col[e];
        if (u < best && sssp_load(d + u) + j.w[e] == dv) best = u;
      }
    }
#pragma unroll
    for (int m = kSsspGroupLanes / 2; m > 0; m >>= 1) {
      const uint32_t o = __shfl_xor(best, m, kSsspGroupLanes);
      if (o < best) best = o;
    }
    if (gl == 0) j.pred[v] = best;
  }
  __syncthreads();
  if (tid == 0) {
    if (j.pred)
      for (uint32_t i = 0; i < j.n_seeds; ++i) {
        const uint32_t v = j.seed_v[i];
        if (j.seed_d[i] == sssp_load(d + v)) j.pred[v] = j.seed_mark;
      }
    if (j.rounds) *j.rounds = rounds;
  }
}

uint32_t sssp_lds_max() {
  uint32_t m = kSsspLdsMaxVertices;
  if (const char* e = getenv("RKH_PRM_PATHS_LDS_MAX")) {
    const long v = atol(e);
    if (v >= 0 && uint64_t(v) < m) m = uint32_t(v);
  }
  return m;
}

rkh_status launch_roadmap_sssp(hipStream_t s, const SsspJob* d_jobs, uint32_t n_jobs, uint32_t n_max) {
  if (n_jobs == 0) return RKH_OK;
  constexpr uint32_t kGridY = 32768;
  const dim3 grid(1, std::min(n_jobs, kGridY), (n_jobs + kGridY - 1) / kGridY);
  if (grid.z > 65535u) {
    set_error("roadmap search: too many searches in one launch");
    return RKH_ERR_CAPACITY;
  }
  if (n_max <= sssp_lds_max()) hipLaunchKernelGGL(roadmap_sssp_kernel<true>, grid, dim3(kSsspThreads), 0, s, d_jobs, n_jobs);
  else hipLaunchKernelGGL(roadmap_sssp_kernel<false>, grid, dim3(kSsspThreads), 0, s, d_jobs, n_jobs);
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

// The comparison side of tools/measure_prm_queries.py: a single-thread std::priority_queue Dijkstra from one vertex.
// Reference code, not the code under test.
void host_dijkstra(const RoadmapCsr& g, uint32_t source, std::vector<double>* dist) {
  typedef std::pair<double, uint32_t> Entry;
  dist->assign(g.n, std::numeric_limits<double>::infinity());
  std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> pq;
  (*dist)[source] = 0.0;
  pq.push(Entry(0.0, source));
  while (!pq.empty()) {
    const Entry t = pq.top();
    pq.pop();
    if (t.first > (*dist)[t.second]) continue;
    for (uint32_t e = g.row_ptr[t.second]; e < g.row_ptr[t.second + 1]; ++e) {
      const double c = t.first + g.w[e];
      if (c < (*dist)[g.col[e]]) {
        (*dist)[g.col[e]] = c;
        pq.push(Entry(c, g.col[e]));
      }
    }
  }
}

}  // namespace rkh

using namespace rkh;

extern "C" {

rkh_status rkh_diag_sssp(rkh_ctx* ctx, uint32_t n, const uint32_t* row_ptr, const uint32_t* col, const double* w, uint32_t S,
                         const uint32_t* seed_ptr, const uint32_t* seed_v, const double* seed_d, const uint32_t* seed_mark,
                         double* dist, uint32_t* pred, uint32_t* rounds) {
  if (!ctx || !row_ptr || n == 0 || (!dist && !pred)) return RKH_ERR_BAD_ARG;
  if (S == 0) return RKH_OK;
  if (!seed_ptr || !seed_mark) return RKH_ERR_BAD_ARG;
  // everything the kernel indexes with is checked here: it trusts its job
  const uint32_t nnz = row_ptr[n], n_seeds = seed_ptr[S];
  bool ok = row_ptr[0] == 0 && seed_ptr[0] == 0 && (nnz == 0 || (col && w)) && (n_seeds == 0 || (seed_v && seed_d));
  for (uint32_t v = 0; ok && v < n; ++v) ok = row_ptr[v] <= row_ptr[v + 1] && row_ptr[v + 1] <= nnz;
  for (uint32_t e = 0; ok && e < nnz; ++e) ok = col[e] < n && w[e] >= 0.0;
  for (uint32_t s = 0; ok && s < S; ++s) ok = seed_ptr[s] <= seed_ptr[s + 1] && seed_ptr[s + 1] <= n_seeds;
  for (uint32_t i = 0; ok && i < n_seeds; ++i) ok = seed_v[i] < n && seed_d[i] >= 0.0;
  if (!ok) {
    set_error("rkh_diag_sssp: malformed CSR or seed lists (offsets must ascend from 0, col and seed vertices < n, weights >= 0)");
    return RKH_ERR_BAD_ARG;
  }
  hipStream_t s = ctx->stream;
  std::vector<SsspJob> jobs(S);  // filled below; declared before the call that uploads it
  StagedCall call(s);
  const uint32_t* d_row = call.in(row_ptr, size_t(n) + 1);
  const uint32_t* d_col = call.in(col, nnz, 1);
  const double* d_w = call.in(w, nnz, 1);
  const uint32_t* d_sv = call.in(seed_v, n_seeds, 1);
  const double* d_sd = call.in(seed_d, n_seeds, 1);
  double* d_dist = call.out(dist, size_t(S) * n);
  uint32_t* d_pred = call.out(pred, size_t(S) * n);
  uint32_t* d_rounds = call.out(rounds, S);
  RKH_TRY(call.status());
  for (uint32_t i = 0; i < S; ++i) {
    SsspJob& j = jobs[i];
    j.row_ptr = d_row;
    j.col = d_col;
    j.w = d_w;
    j.n = n;
    j.n_seeds = seed_ptr[i + 1] - seed_ptr[i];
    j.seed_v = d_sv + seed_ptr[i];
    j.seed_d = d_sd + seed_ptr[i];
    j.seed_mark = seed_mark[i];
    j.dist = d_dist + size_t(i) * n;
    j.pred = d_pred + size_t(i) * n;
    j.rounds = d_rounds + i;
  }
  const SsspJob* d_jobs = call.in(jobs.data(), S);
  RKH_TRY(call.status());
  RKH_TRY(launch_roadmap_sssp(s, d_jobs, S, n));
  return call.fetch();
}

}  // extern "C"
