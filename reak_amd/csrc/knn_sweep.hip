// knn_sweep.hip -- exact batched k-nearest-neighbour (with radius) sweeps over the tree (gfx950).
//
// Replaces min_dist_linear_search k-NN (ctrl/path_planning/topological_search.hpp:244-274: bounded max-heap,
// candidates need d < radius strictly, output ascending) with euclidean_distance_metric
// (ctrl/topologies/vect_distance_metrics.hpp:113-150), as used by star_neighborhood
// (ctrl/graph_alg/neighborhood_functors.hpp:95-102) for RRT* / PRM.
//
// A per-thread top-k does not fit registers (k = 4(floor(log2 n)+1) = 84 at n = 1M), so the search is
//   A. bound sweep   : every thread keeps only the minimum of its own row subset; the k-th smallest of those
//                      M = blocks x R subset minima is an upper bound tau on the k-th smallest distance overall
//                      (k disjoint subsets each hold a vertex at least that close)
//   B. collect sweep : every vertex with d <= tau and d < radius is appended to the query's candidate list
//                      (about 1.2 k entries when M >= 4k); exact: the true k nearest are all in the list
//   C. select        : one block per query sorts its candidates by (distance, index) and writes the first k.
// tau is a bound, not a promise (fewer than k finite subset minima: tau = +inf): a query whose list of cmax slots
// overflowed is answered by the EXACT RETRY (knn_exact_tau_kernel below, then B and C again for that query alone),
// which the callers launch only after they have seen the overflow word set (knn_plan.h: the guarantee).
// Distances are the reference's left-to-right fp64 sums with a correctly rounded sqrt, so the returned set and
// its order equal the CPU search's (among exactly equal distances the reference order is std::heap-defined; here
// it is ascending index).  Same tile / broadcast structure as nn_sweep.hip; traffic is two passes over the rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>

#include "nn_device.h"
#include "rkh_internal.h"

namespace rkh {

int nn_padded_dims(int D);

// the launch shape (gx, ksel, m_sub, cmax), the workspace and what the plan guarantees: knn_plan.h
static constexpr int kTileRows = kKnnTileRows;
static constexpr int kThreads = kKnnThreads;

// MODE 0: bound sweep (per query, the kSel smallest of the block's R = 256/QB row-subset minima).
// MODE 1: collect sweep (appends candidates).
// Thread (ql, r) keeps query ql in registers and scans rows r, r+R, .. of every tile; with few queries (RRT* / PRM:
// one per tree) QB = 8 puts 32 threads on each query so the whole block works on the rows.  The next tile is fetched
// into registers while the current one is scanned (as in nn_sweep.hip).
template <int DP, int QB, int MODE>
__global__ __launch_bounds__(kThreads) void knn_sweep_kernel(KnnArgs single, const KnnArgs* __restrict__ tab) {
  constexpr int R = kThreads / QB;
  constexpr int ROWS_PER_THREAD = kTileRows / R;
  const KnnArgs a = tab ? tab[blockIdx.z] : single;
  if (blockIdx.x >= a.ws.gx || blockIdx.y * QB >= a.B) return;  // a table's grid is sized for its largest job
  const double* __restrict__ pos = a.pos;
  const uint64_t n = a.n;
  const double* __restrict__ q = a.q;
  const int D = a.D;
  const uint32_t B = a.B, Bpad = a.B, cmax = a.ws.cmax;
  const double radius = a.radius;
  double* __restrict__ sub = a.ws.sub;
  const double* __restrict__ tau = a.ws.tau;
  uint32_t* __restrict__ cnt = a.ws.cnt;
  double* __restrict__ cand_d = a.ws.cand_d;
  uint32_t* __restrict__ cand_i = a.ws.cand_i;
  uint32_t* __restrict__ overflow = a.ws.overflow;
  const uint32_t gx = a.ws.gx;
  __shared__ __attribute__((aligned(16))) double tile[kTileRows * DP];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int ql = tid % QB;
  const int r = tid / QB;
  const uint32_t qi = blockIdx.y * QB + ql;
  const bool q_valid = qi < B;
  double qv[DP];
  {
    const uint64_t qsrc = q_valid ? qi : (B - 1);
#pragma unroll
    for (int d = 0; d < DP; ++d) qv[d] = d < D ? q[qsrc * D + d] : 0.0;
  }
  const uint64_t tiles_total = (n + kTileRows - 1) / kTileRows;
  const uint64_t tiles_per_block = (tiles_total + gx - 1) / gx;
  const uint64_t tile0 = uint64_t(blockIdx.x) * tiles_per_block;
  uint64_t tile1 = tile0 + tiles_per_block;
  if (tile1 > tiles_total) tile1 = tiles_total;

  double best_s = INFINITY;  // MODE 0: smallest square of this thread's subset
  double t_q = INFINITY, thr_s = INFINITY;
  if (MODE == 1) {
    t_q = tau[q_valid ? qi : 0];
    // squares above this cannot give sqrt(s) <= tau (4 ulp of slack for the rounding of tau*tau and of sqrt)
    thr_s = (t_q == INFINITY) ? INFINITY : (t_q * t_q) * (1.0 + 8.0 * DBL_EPSILON);
  }
  constexpr int N2 = kTileRows * DP / 2;
  constexpr int PF = N2 / kThreads;
  static_assert(N2 % kThreads == 0, "tile must split evenly");
  double2 pf[PF];
  auto fetch = [&](uint64_t t) {
    const uint64_t row_base = t * kTileRows;
    const double2* src = reinterpret_cast<const double2*>(pos + row_base * DP);
    const uint64_t valid2 = (n - row_base >= uint64_t(kTileRows)) ? uint64_t(N2) : (n - row_base) * DP / 2;
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int i = tid + j * kThreads;
      pf[j] = (uint64_t(i) < valid2) ? src[i] : make_double2(INFINITY, INFINITY);  // rows beyond n never qualify
    }
  };
  if (tile0 < tile1) fetch(tile0);
  for (uint64_t t = tile0; t < tile1; ++t) {
    const uint64_t row_base = t * kTileRows;
    {
      double2* dst = reinterpret_cast<double2*>(tile);
#pragma unroll
      for (int j = 0; j < PF; ++j) dst[tid + j * kThreads] = pf[j];
    }
    if (t + 1 < tile1) fetch(t + 1);
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < ROWS_PER_THREAD; ++k) {
      const int row = k * R + r;
      const double* p = tile + row * DP;
      const double s = nn_exact_sq<DP>([&](int d) { return qv[d] - p[d]; });
      if (MODE == 0) {
        if (s < best_s) best_s = s;
      } else if (s <= thr_s && q_valid) {
        const double dd = sqrt(s);
        if (dd <= t_q && dd < radius) {
          const uint32_t slot = atomicAdd(&cnt[qi], 1u);
          if (slot < cmax) {
            cand_d[uint64_t(qi) * cmax + slot] = dd;
            cand_i[uint64_t(qi) * cmax + slot] = uint32_t(row_base + row);
          } else {
            *overflow = 1u;
          }
        }
      }
    }
    __syncthreads();
  }
  if (MODE == 0) {
    // the ksel smallest of the R subset minima of every query (ranks by (value, subset) are a permutation; any k
    // disjoint subsets with minimum <= tau prove that k vertices lie within tau, so dropping the larger ones is safe)
    const double mine = sqrt(best_s);
    red[tid] = mine;
    __syncthreads();
    int rank = 0;
#pragma unroll 8
    for (int rr = 0; rr < R; ++rr) {
      const double v = red[rr * QB + ql];
      rank += (v < mine || (v == mine && rr < r)) ? 1 : 0;
    }
    const int ksel = int(a.ws.ksel);
    if (q_valid && rank < ksel) sub[(uint64_t(blockIdx.x) * ksel + rank) * Bpad + qi] = mine;
  }
}

// bitonic sort of (key, idx) pairs in LDS, ascending lexicographic; n_pow2 elements, blockDim.x threads
__device__ __forceinline__ void bitonic_sort_lds(double* key, uint32_t* idx, uint32_t n_pow2) {
  for (uint32_t size = 2; size <= n_pow2; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < n_pow2 / 2; t += blockDim.x) {
        const uint32_t lo = 2 * t - (t & (stride - 1));
        const uint32_t hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const double ka = key[lo], kb = key[hi];
        const uint32_t ia = idx[lo], ib = idx[hi];
        const bool a_gt_b = (ka > kb) || (ka == kb && ia > ib);
        if (a_gt_b == up) {
          key[lo] = kb; key[hi] = ka;
          idx[lo] = ib; idx[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
}

// one block per query: tau = k-th smallest subset minimum (or +inf if there are fewer than k subsets)
__global__ __launch_bounds__(256) void knn_tau_kernel(KnnArgs single, const KnnArgs* __restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KnnArgs a = tab ? tab[blockIdx.z] : single;
  const uint32_t qi = blockIdx.x;
  if (qi >= a.B) return;
  const double* __restrict__ sub = a.ws.sub;
  const uint32_t m_sub = a.ws.m_sub, m_pow2 = a.m_pow2, Bpad = a.B, k = a.k;
  double* __restrict__ tau = a.ws.tau;
  uint32_t* __restrict__ cnt = a.ws.cnt;
  uint32_t* __restrict__ overflow = a.ws.overflow;
  double* key = reinterpret_cast<double*>(smem);
  uint32_t* idx = reinterpret_cast<uint32_t*>(key + m_pow2);
  for (uint32_t i = threadIdx.x; i < m_pow2; i += blockDim.x) {
    key[i] = i < m_sub ? sub[uint64_t(i) * Bpad + qi] : INFINITY;
    idx[i] = i;
  }
  bitonic_sort_lds(key, idx, m_pow2);
  if (threadIdx.x == 0) {
    tau[qi] = (m_sub >= k) ? key[k - 1] : INFINITY;
    cnt[qi] = 0;
    if (qi == 0) *overflow = 0;
  }
}

// one block per query: sort the candidates, write the first k (nearest first), pad the rest
__global__ __launch_bounds__(256) void knn_select_kernel(KnnArgs single, const KnnArgs* __restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KnnArgs a = tab ? tab[blockIdx.z] : single;
  const uint32_t qi = blockIdx.x;
  if (qi >= a.B) return;
  const double* __restrict__ cand_d = a.ws.cand_d;
  const uint32_t* __restrict__ cand_i = a.ws.cand_i;
  const uint32_t* __restrict__ cnt = a.ws.cnt;
  const uint32_t cmax = a.ws.cmax, c_pow2 = a.ws.cmax, k = a.k;
  uint32_t* __restrict__ out_idx = a.out_idx;
  double* __restrict__ out_dist = a.out_dist;
  uint32_t* __restrict__ out_cnt = a.out_cnt;
  double* key = reinterpret_cast<double*>(smem);
  uint32_t* idx = reinterpret_cast<uint32_t*>(key + c_pow2);
  uint32_t nc = cnt[qi];
  if (nc > cmax) nc = cmax;
  uint32_t n_sort = 1;  // sort only as many slots as there are candidates (power of two, <= c_pow2)
  while (n_sort < nc) n_sort <<= 1;
  for (uint32_t i = threadIdx.x; i < n_sort; i += blockDim.x) {
    key[i] = i < nc ? cand_d[uint64_t(qi) * cmax + i] : INFINITY;
    idx[i] = i < nc ? cand_i[uint64_t(qi) * cmax + i] : 0xFFFFFFFFu;
  }
  bitonic_sort_lds(key, idx, n_sort);
  const uint32_t found = nc < k ? nc : k;
  for (uint32_t i = threadIdx.x; i < k; i += blockDim.x) {
    out_idx[uint64_t(qi) * k + i] = i < found ? idx[i] : 0xFFFFFFFFu;
    out_dist[uint64_t(qi) * k + i] = i < found ? key[i] : INFINITY;
  }
  if (threadIdx.x == 0) out_cnt[qi] = found;
}

// THE EXACT RETRY (knn_plan.h, the guarantee).  One block per query, after a first pass: a query whose list overflowed
// (cnt > cmax) gets tau = the k-th smallest distance among the vertices with d < radius, found by bisection over the bit
// patterns of the non-negative doubles -- 63 counting passes over the rows, no list, the same nn_exact_sq and sqrt as
// the sweeps, so the bound is the very number the collect sweep compares with -- and an empty list; every other query
// gets tau = -1, which no distance is below: the collect sweep that follows appends nothing to its list and the select
// kernel writes its result again as it was.  Fewer than k vertices inside the radius: tau = +inf (they all fit).
template <int DP>
__global__ __launch_bounds__(kThreads) void knn_exact_tau_kernel(KnnArgs single, const KnnArgs* __restrict__ tab) {
  const KnnArgs a = tab ? tab[blockIdx.z] : single;
  const uint32_t qi = blockIdx.x;
  if (qi >= a.B) return;
  const int tid = threadIdx.x;
  const bool redo = a.ws.cnt[qi] > a.ws.cmax;  // the same for the whole block
  if (tid == 0 && qi == 0) *a.ws.overflow = 0;  // nobody sets it before the collect sweep
  if (!redo) {
    if (tid == 0) a.ws.tau[qi] = -1.0;
    return;
  }
  const double* __restrict__ pos = a.pos;
  const uint64_t n = a.n;
  const double radius = a.radius;
  __shared__ uint32_t red[kThreads];
  double qv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) qv[d] = d < a.D ? a.q[uint64_t(qi) * a.D + d] : 0.0;
  // vertices with d <= t and d < radius (the same value in every thread)
  auto count_le = [&](double t) -> uint32_t {
    uint32_t c = 0;
    for (uint64_t row = tid; row < n; row += kThreads) {
      const double* p = pos + row * DP;
      const double dd = sqrt(nn_exact_sq<DP>([&](int d) { return qv[d] - p[d]; }));
      c += (dd <= t && dd < radius) ? 1u : 0u;
    }
    red[tid] = c;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    const uint32_t total = red[0];
    __syncthreads();
    return total;
  };
  double t = INFINITY;
  if (count_le(INFINITY) >= a.k) {
    // every counted distance is finite (d < radius <= +inf): the answer is the smallest bit pattern with count >= k
    unsigned long long lo = 0ull, hi = 0x7FEFFFFFFFFFFFFFull;  // +0 .. DBL_MAX
    while (lo < hi) {
      const unsigned long long mid = lo + (hi - lo) / 2;
      if (count_le(__longlong_as_double((long long)mid)) >= a.k) hi = mid;
      else lo = mid + 1;
    }
    t = __longlong_as_double((long long)lo);
  }
  if (tid == 0) {
    a.ws.tau[qi] = t;
    a.ws.cnt[qi] = 0;
  }
}

struct KnnGrid {  // the grid of one job, or the largest of a table's jobs
  uint32_t gx = 0, gy = 0, b_max = 0, m_pow2 = 0, cmax = 0, n_jobs = 0;
};

template <int DP>
static void launch_nnk_dp(hipStream_t s, const KnnArgs& single, const KnnArgs* d_tab, const KnnGrid& g, bool retry) {
  dim3 grid(g.gx, g.gy, g.n_jobs), block(kThreads), per_query(g.b_max, 1, g.n_jobs);
  const bool few = knn_query_block(g.b_max) == 8;
  if (!retry) {
    if (few) hipLaunchKernelGGL((knn_sweep_kernel<DP, 8, 0>), grid, block, 0, s, single, d_tab);
    else hipLaunchKernelGGL((knn_sweep_kernel<DP, 32, 0>), grid, block, 0, s, single, d_tab);
    hipLaunchKernelGGL(knn_tau_kernel, per_query, dim3(256), size_t(g.m_pow2) * 12, s, single, d_tab);
  } else {
    hipLaunchKernelGGL(knn_exact_tau_kernel<DP>, per_query, block, 0, s, single, d_tab);
  }
  if (few) hipLaunchKernelGGL((knn_sweep_kernel<DP, 8, 1>), grid, block, 0, s, single, d_tab);
  else hipLaunchKernelGGL((knn_sweep_kernel<DP, 32, 1>), grid, block, 0, s, single, d_tab);
  hipLaunchKernelGGL(knn_select_kernel, per_query, dim3(256), size_t(g.cmax) * 12, s, single, d_tab);
}

static std::atomic<uint64_t> g_knn_retries{0};
uint64_t knn_retry_count() { return g_knn_retries.load(std::memory_order_relaxed); }

uint32_t knn_list_cap_from_env() {
  const char* e = getenv("RKH_KNN_LIST_CAP");
  return e ? uint32_t(std::max(0, atoi(e))) : 0u;
}

static rkh_status launch_nnk_any(hipStream_t s, int D, const KnnArgs& single, const KnnArgs* d_tab, const KnnGrid& g,
                                 bool retry) {
  if (retry) g_knn_retries.fetch_add(1, std::memory_order_relaxed);
  const bool dims_ok = with_padded_dims(D, [&](auto dp) {
    launch_nnk_dp<decltype(dp)::value>(s, single, d_tab, g, retry);
  });
  if (!dims_ok) {
    set_error("k-NN: unsupported dimension");
    return RKH_ERR_BAD_ARG;
  }
  RKH_HIP(hipGetLastError());
  return RKH_OK;
}

static rkh_status launch_nnk_one(hipStream_t s, const NnStore& st, uint64_t n, const double* d_q, uint32_t B, uint32_t k,
                                 double radius, uint32_t* d_idx, double* d_dist, uint32_t* d_count, const KnnWorkspace& ws,
                                 bool retry) {
  if (B == 0) return RKH_OK;
  KnnArgs a;
  a.pos = st.d_pos;
  a.n = n;
  a.q = d_q;
  a.D = st.D;
  a.B = B;
  a.k = k;
  a.radius = radius;
  a.ws = ws;
  a.m_pow2 = next_pow2(ws.m_sub);
  a.out_idx = d_idx;
  a.out_dist = d_dist;
  a.out_cnt = d_count;
  KnnGrid g;
  g.gx = ws.gx;
  g.gy = (B + knn_query_block(B) - 1) / knn_query_block(B);
  g.b_max = B;
  g.m_pow2 = a.m_pow2;
  g.cmax = ws.cmax;
  g.n_jobs = 1;
  return launch_nnk_any(s, st.D, a, nullptr, g, retry);
}

rkh_status launch_nnk(hipStream_t s, const NnStore& st, uint64_t n, const double* d_q, uint32_t B, uint32_t k,
                      double radius, uint32_t* d_idx, double* d_dist, uint32_t* d_count, const KnnWorkspace& ws) {
  return launch_nnk_one(s, st, n, d_q, B, k, radius, d_idx, d_dist, d_count, ws, false);
}

rkh_status launch_nnk_retry(hipStream_t s, const NnStore& st, uint64_t n, const double* d_q, uint32_t B, uint32_t k,
                            double radius, uint32_t* d_idx, double* d_dist, uint32_t* d_count, const KnnWorkspace& ws) {
  return launch_nnk_one(s, st, n, d_q, B, k, radius, d_idx, d_dist, d_count, ws, true);
}

static rkh_status launch_nnk_jobs(hipStream_t s, int D, const KnnArgs* d_table, const KnnArgs* h_table, uint32_t n_jobs,
                                  bool retry) {
  KnnGrid g;
  for (uint32_t i = 0; i < n_jobs; ++i) {
    const KnnArgs& a = h_table[i];
    if (a.B == 0) continue;
    g.gx = std::max(g.gx, a.ws.gx);
    g.b_max = std::max(g.b_max, a.B);
    g.m_pow2 = std::max(g.m_pow2, a.m_pow2);
    g.cmax = std::max(g.cmax, a.ws.cmax);
  }
  if (g.b_max == 0) return RKH_OK;
  g.gy = (g.b_max + knn_query_block(g.b_max) - 1) / knn_query_block(g.b_max);
  g.n_jobs = n_jobs;
  return launch_nnk_any(s, D, KnnArgs(), d_table, g, retry);
}

rkh_status launch_nnk_table(hipStream_t s, int D, const KnnArgs* d_table, const KnnArgs* h_table, uint32_t n_jobs) {
  return launch_nnk_jobs(s, D, d_table, h_table, n_jobs, false);
}

rkh_status launch_nnk_table_retry(hipStream_t s, int D, const KnnArgs* d_table, const KnnArgs* h_table, uint32_t n_jobs) {
  return launch_nnk_jobs(s, D, d_table, h_table, n_jobs, true);
}

}  // namespace rkh
