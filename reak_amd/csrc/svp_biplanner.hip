// svp_biplanner.hip -- batch bidirectional RRT over the order-1 rate-limited joint space with SVP profiles
// (rkh_svp_birrt_*, rkh.h): P problems on one scene, each with a tree rooted at its start that grows forward and a tree
// rooted at its goal that grows backward (the edge of a goal-tree vertex v is the profile v -> parent(v)); trees, sample
// streams and per-problem state live in one arena on the device.  Each problem's two trees are those of the sequential
// loop rkh.h states (tests/svp_birrt_ref.py), bit for bit: the arithmetic is svp_device.h's, the scalar rules are
// svp_rrt_device.h's, the walk is svp_walk_dir.hip's.
//
// A round is one half step of every live problem; each problem keeps its own side, so one launch holds both directions:
//   rl1bi_sample_kernel    one block per live problem, at work only where the pending target is none: the window / refill /
//                          skip-rejected scheme of the RRT's sample kernel (restated here: that kernel's text is pinned by
//                          its resource table); at most 16 refills a launch, a problem that found none sits the round out
//   rl1bi_nearest_kernel   one block per (slice of 256 vertices of the side's tree, live problem): d(vertex -> target) on
//                          side 0, d(target -> vertex) on side 1; the reduction of the RRT's nearest kernel
//   rl1bi_steer_kernel     one lane per live problem: merges the slices' minima (ties to the lower index), the steer
//                          fraction, the walk's row and its direction byte
//   [walk: launch_svp_walk_dir, once]
//   rl1bi_commit_kernel    one lane per live problem: the join, the progress rule, the append, the other side's next target,
//                          the flip of the side, the end conditions in the loop's order, the next round's live list and the
//                          record the host reads back (one small copy per round)
// Problems without work in the walk ride as the row (start, start, fraction 0), forward: no point to test.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "rkh_internal.h"
#include "svp_device.h"
#include "svp_rrt_device.h"

namespace rkh {
namespace {

constexpr uint32_t kBiThreads = 256;
constexpr uint32_t kBiSlice = 256;            // vertices per block of the nearest sweep: one pair per lane
constexpr uint32_t kBiWindow = 64;            // candidates generated ahead of a problem's cursor
constexpr uint32_t kBiRefillsPerLaunch = 16;  // a launch of the sample kernel draws at most 1024 candidates per problem
constexpr uint32_t kBiMaxProblems = 16384;
constexpr uint32_t kNone = 0xFFFFFFFFu;

enum : uint32_t { kRunning = 0, kJoined = 1, kMaxVertices = 2, kMaxIterations = 3 };
// BiProblem::step within a round.  kIdle: no half step (no candidate found in this launch's refills); kNoNeighbour: a half
// step without a finite distance; kExtend: a half step with a walk row
enum : uint32_t { kIdle = 0, kExtend = 1, kNoNeighbour = 2 };

struct BiProblem {  // one problem on the device
  double max_edge_time, steer_tol;
  double start[2 * kSvpMaxDof], goal[2 * kSvpMaxDof];
  double asked, fraction, join_time;
  uint64_t v_off;  // first row of tree 0 in the shared vertex arrays; tree 1 starts max_vertices rows later
  uint32_t seed, max_vertices, max_iterations;
  uint32_t n[2], iterations, join0, join1, status;
  uint32_t side;      // the tree the next half step grows
  uint32_t target_v;  // the pending target's vertex in the other tree (its point is q[p]); kNone: a sample is needed
  uint32_t win_end;   // candidates generated so far: the window holds [win_end - 64, win_end)
  uint32_t refills;
  uint32_t step, nn_idx;
};

struct BiRecord {  // what the host reads back after a round
  uint32_t live_cnt[2];
  uint32_t finished, max_n;
  unsigned long long iterations, vertices, tested, refills;
};

struct BiDev {  // device pointers into the planner's arena, by value
  BiProblem* prob;    // [P]
  uint32_t* mt;       // [P][624 + 1] generator state + position
  double* window;     // [P][64][2n]
  uint8_t* verdict;   // [P][64]
  double* q;          // [P][2n] the half step's target point
  double* part_d;     // [P][slices]
  uint32_t* part_i;
  double* verts;      // [2 sum max_vertices][2n]
  uint32_t* parent;   // [2 sum max_vertices]
  double* etime;
  uint8_t* back;      // [P] the walk rows' direction bytes
  uint32_t* live[2];  // [P]
  BiRecord* rec;
  uint32_t slices;    // ceil(largest max_vertices / 256)
};

__device__ __forceinline__ bool bi_less(double d1, uint32_t i1, double d2, uint32_t i2) {
  return (d1 < d2) || (d1 == d2 && i1 < i2);
}

__device__ __forceinline__ uint64_t bi_tree_row(const BiProblem& st, uint32_t side) {
  return st.v_off + uint64_t(side) * st.max_vertices;
}

// the walk row of a problem without work: nothing to solve, nothing to test
__device__ __forceinline__ void bi_idle_row(const SvpWalk& w, uint8_t* back, uint32_t l, const double* x, uint32_t D) {
  double* a = const_cast<double*>(w.a) + size_t(l) * D;
  double* b = const_cast<double*>(w.b) + size_t(l) * D;
  for (uint32_t c = 0; c < D; ++c) a[c] = x[c], b[c] = x[c];
  const_cast<double*>(w.fraction)[l] = 0.0;
  back[l] = 0;
}

// grid (P).  The arena may have served another planner: whatever a kernel reads before a kernel writes it is written here.
// A problem whose trees are full with their roots (max_vertices 1) has ended before its first half step.
__global__ __launch_bounds__(256) void rl1bi_init_kernel(const SvpDev sp, const BiDev pl) {
  const uint32_t p = blockIdx.x, tid = threadIdx.x;
  BiProblem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  if (tid < D) {
    pl.verts[bi_tree_row(st, 0) * D + tid] = st.start[tid];
    pl.verts[bi_tree_row(st, 1) * D + tid] = st.goal[tid];
    pl.q[size_t(p) * D + tid] = st.goal[tid];  // the first half step is the attempt start -> goal
  }
  if (tid == 64) {
    for (uint32_t side = 0; side < 2; ++side) {
      pl.parent[bi_tree_row(st, side)] = kNone;
      pl.etime[bi_tree_row(st, side)] = 0.0;
    }
    st.n[0] = 1, st.n[1] = 1, st.iterations = 0, st.join0 = kNone, st.join1 = kNone, st.join_time = 0.0;
    st.side = 0, st.target_v = 0;
    st.win_end = 0, st.refills = 0, st.step = kIdle, st.nn_idx = 0, st.asked = 0.0, st.fraction = 0.0;
    if (st.max_vertices <= 1) {
      st.status = kMaxVertices;
      atomicAdd(&pl.rec->finished, 1u);
    } else {
      st.status = kRunning;
      pl.live[0][atomicAdd(&pl.rec->live_cnt[0], 1u)] = p;
    }
  }
  if (tid == 128) {
    uint32_t* mt = pl.mt + size_t(p) * (kRl1MtN + 1);
    uint32_t v = st.seed;
    mt[0] = v;
    for (uint32_t k = 1; k < kRl1MtN; ++k) {
      v = rl1rrt_mt_seed_next(v, k);
      mt[k] = v;
    }
    mt[kRl1MtN] = kRl1MtN;
  }
}

// grid (L).  See the head of the file.
__global__ __launch_bounds__(256) void rl1bi_sample_kernel(const SvpDev sp, const BiDev pl, uint32_t cur) {
  __shared__ uint32_t mt[kRl1MtN];
  __shared__ uint32_t first;
  const uint32_t tid = threadIdx.x;
  const uint32_t p = pl.live[cur][blockIdx.x];
  BiProblem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  const uint32_t it0 = st.iterations, max_it = st.max_iterations;
  const bool pending = st.target_v != kNone;
  uint32_t it = it0, win_end = st.win_end;
  __syncthreads();  // everybody has read the state lane 0 writes
  if (pending || it0 >= max_it) {  // uniform.  (a live problem without a target has iterations left: the commit ends the others)
    if (tid == 0) st.step = pending ? kExtend : kIdle;
    return;
  }
  double* const win = pl.window + size_t(p) * kBiWindow * D;
  uint8_t* const ok = pl.verdict + size_t(p) * kBiWindow;
  uint32_t* const g_mt = pl.mt + size_t(p) * (kRl1MtN + 1);
  uint32_t found = kNone, refills = 0, idx = 0;
  bool loaded = false;
  while (true) {  // uniform
    if (it == win_end) {
      if (!loaded) {
        for (uint32_t i = tid; i < kRl1MtN; i += kBiThreads) mt[i] = g_mt[i];
        idx = g_mt[kRl1MtN];
        loaded = true;
        __syncthreads();
      }
      const uint32_t count = kBiWindow * D;
      uint32_t produced = 0;
      while (produced < count) {
        if (idx == kRl1MtN) {
          // words [a, b): new[i] = twist(old[i], old[i + 1], word (i + 397) mod 624 as it stands at this point)
          auto stretch = [&](uint32_t a, uint32_t b) {
            const uint32_t i = a + tid;
            uint32_t v = 0;
            if (i < b) v = rl1rrt_mt_twist(mt[i], mt[i + 1], mt[i + kRl1MtM < kRl1MtN ? i + kRl1MtM : i + kRl1MtM - kRl1MtN]);
            __syncthreads();  // every thread has read its old neighbour before anybody overwrites it
            if (i < b) mt[i] = v;
            __syncthreads();
          };
          stretch(0, kRl1MtN - kRl1MtM);                        // 0 .. 226
          stretch(kRl1MtN - kRl1MtM, 2 * (kRl1MtN - kRl1MtM));  // 227 .. 453
          stretch(2 * (kRl1MtN - kRl1MtM), kRl1MtN - 1);        // 454 .. 622
          if (tid == 0) mt[kRl1MtN - 1] = rl1rrt_mt_twist(mt[kRl1MtN - 1], mt[0], mt[kRl1MtM - 1]);
          __syncthreads();
          idx = 0;
        }
        const uint32_t left = count - produced;
        const uint32_t chunk = (kRl1MtN - idx < left) ? kRl1MtN - idx : left;
        for (uint32_t t = tid; t < chunk; t += kBiThreads) {
          const double u = rl1rrt_unit(rl1rrt_mt_temper(mt[idx + t]));
          double lo, hi;
          rl1rrt_coord_range(sp, (produced + t) % D, &lo, &hi);
          win[produced + t] = rl1rrt_coord(lo, hi, u);
        }
        produced += chunk;
        idx += chunk;
        __syncthreads();
      }
      if (tid < kBiWindow) ok[tid] = svp_in_bounds(sp, win + size_t(tid) * D) ? 1 : 0;
      __syncthreads();
      win_end += kBiWindow;
      ++refills;
    }
    const uint32_t avail = win_end - it, left_it = max_it - it;
    const uint32_t lim = avail < left_it ? avail : left_it;  // 1 .. 64
    const uint32_t slot0 = kBiWindow - avail;
    if (tid == 0) first = lim;
    __syncthreads();
    if (tid < lim && ok[slot0 + tid]) atomicMin(&first, tid);
    __syncthreads();
    const uint32_t f = first;
    __syncthreads();
    if (f < lim) {
      found = slot0 + f;
      it += f + 1;
      break;
    }
    it += lim;
    if (it == max_it) break;
    // a box that rejects (nearly) everything: the problem sits this round out and draws on in the next
    if (refills >= kBiRefillsPerLaunch) break;
  }
  if (loaded) {
    for (uint32_t i = tid; i < kRl1MtN; i += kBiThreads) g_mt[i] = mt[i];
    if (tid == 0) g_mt[kRl1MtN] = idx;
  }
  if (found != kNone && tid < D) pl.q[size_t(p) * D + tid] = win[size_t(found) * D + tid];
  if (tid == 0) {
    st.iterations = it, st.win_end = win_end, st.refills += refills;
    st.step = found != kNone ? kExtend : kIdle;
    atomicAdd(&pl.rec->iterations, (unsigned long long)(it - it0));
    if (refills) atomicAdd(&pl.rec->refills, (unsigned long long)refills);
  }
}

// grid (slices of the largest live tree, L)
__global__ __launch_bounds__(256) void rl1bi_nearest_kernel(const SvpDev sp, const BiDev pl, uint32_t cur) {
  __shared__ double qv[2 * kSvpMaxDof];
  __shared__ double red_d[kBiThreads / 64];
  __shared__ uint32_t red_i[kBiThreads / 64];
  const uint32_t tid = threadIdx.x, s = blockIdx.x;
  const uint32_t p = pl.live[cur][blockIdx.y];
  const BiProblem& st = pl.prob[p];
  const uint32_t side = st.side;
  const uint32_t n = st.n[side], base = s * kBiSlice;
  if (st.step != kExtend || base >= n) return;  // uniform
  const uint32_t D = 2 * uint32_t(sp.n);
  if (tid < D) qv[tid] = pl.q[size_t(p) * D + tid];
  __syncthreads();
  const uint32_t g = base + tid;
  double d = INFINITY;
  uint32_t i = kNone;
  if (g < n) {
    const double* v = pl.verts + (bi_tree_row(st, side) + g) * D;
    d = side ? svp_reach(sp, qv, v, nullptr) : svp_reach(sp, v, qv, nullptr);
    i = g;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const double od = __shfl_xor(d, m, 64);
    const uint32_t oi = __shfl_xor(i, m, 64);
    if (bi_less(od, oi, d, i)) d = od, i = oi;
  }
  if ((tid & 63) == 0) red_d[tid >> 6] = d, red_i[tid >> 6] = i;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < kBiThreads / 64; ++w)
      if (bi_less(red_d[w], red_i[w], d, i)) d = red_d[w], i = red_i[w];
    pl.part_d[size_t(p) * pl.slices + s] = d;
    pl.part_i[size_t(p) * pl.slices + s] = i;
  }
}

// one lane per live problem
__global__ __launch_bounds__(256) void rl1bi_steer_kernel(const SvpDev sp, const BiDev pl, const SvpWalk w, uint32_t cur,
                                                          uint32_t L) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint32_t p = pl.live[cur][l];
  BiProblem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  if (st.step != kExtend) {
    bi_idle_row(w, pl.back, l, st.start, D);
    return;
  }
  const uint32_t side = st.side;
  double d = INFINITY;
  uint32_t i = kNone;
  const uint32_t ns = (st.n[side] + kBiSlice - 1) / kBiSlice;
  for (uint32_t s = 0; s < ns; ++s) {  // ascending slices hold ascending indices: "less" keeps the lower one of a tie
    const double sd = pl.part_d[size_t(p) * pl.slices + s];
    if (sd < d) d = sd, i = pl.part_i[size_t(p) * pl.slices + s];
  }
  if (!(d < INFINITY)) {
    st.step = kNoNeighbour;
    bi_idle_row(w, pl.back, l, st.start, D);
    return;
  }
  const double f = rl1rrt_fraction(d, st.max_edge_time);
  st.nn_idx = i, st.asked = d, st.fraction = f;
  const double* v = pl.verts + (bi_tree_row(st, side) + i) * D;
  const double* q = pl.q + size_t(p) * D;
  double* a = const_cast<double*>(w.a) + size_t(l) * D;
  double* b = const_cast<double*>(w.b) + size_t(l) * D;
  if (side == 0)
    for (uint32_t c = 0; c < D; ++c) a[c] = v[c], b[c] = q[c];
  else  // the profile target -> vertex, walked from the vertex backward
    for (uint32_t c = 0; c < D; ++c) a[c] = q[c], b[c] = v[c];
  const_cast<double*>(w.fraction)[l] = f;
  pl.back[l] = uint8_t(side);
}

// one lane per live problem, after the walk
__global__ __launch_bounds__(256) void rl1bi_commit_kernel(const SvpDev sp, const BiDev pl, const SvpWalk w, uint32_t cur,
                                                           uint32_t L) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint32_t p = pl.live[cur][l];
  BiProblem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  const uint32_t step = st.step, side = st.side;
  uint32_t status = kRunning;
  if (step != kIdle) {  // a half step
    uint32_t moved = kNone;
    const double* out = w.out + size_t(l) * D;
    if (step == kExtend) {
      const uint32_t nc = w.n_checked[l];
      if (nc) atomicAdd(&pl.rec->tested, (unsigned long long)nc);
      if (st.target_v != kNone && st.fraction == 1.0 && w.reached[l]) {
        st.join0 = side == 0 ? st.nn_idx : st.target_v;
        st.join1 = side == 0 ? st.target_v : st.nn_idx;
        st.join_time = st.asked;
        status = kJoined;
      } else if (nc) {
        const double* a = w.a + size_t(l) * D;
        const double* b = w.b + size_t(l) * D;
        const double travelled = side == 0 ? svp_reach(sp, a, out, nullptr) : svp_reach(sp, out, b, nullptr);
        if (rl1rrt_progress(travelled, st.asked, st.fraction, st.steer_tol)) {
          const uint32_t v = st.n[side];
          const uint64_t r = bi_tree_row(st, side) + v;
          double* row = pl.verts + r * D;
          for (uint32_t c = 0; c < D; ++c) row[c] = out[c];
          pl.parent[r] = st.nn_idx;
          pl.etime[r] = travelled;
          st.n[side] = v + 1;
          atomicAdd(&pl.rec->vertices, 1ull);
          atomicMax(&pl.rec->max_n, v + 1);
          moved = v;
        }
      }
    }
    if (status == kRunning) {
      st.target_v = moved;
      if (moved != kNone) {
        double* q = pl.q + size_t(p) * D;
        for (uint32_t c = 0; c < D; ++c) q[c] = out[c];
      }
      st.side = 1 - side;
    }
  }
  st.step = kIdle;
  // the top of the loop
  if (status == kRunning) {
    if (st.n[0] >= st.max_vertices || st.n[1] >= st.max_vertices) status = kMaxVertices;
    else if (st.target_v == kNone && st.iterations >= st.max_iterations) status = kMaxIterations;
  }
  st.status = status;
  if (status == kRunning) pl.live[1 - cur][atomicAdd(&pl.rec->live_cnt[1 - cur], 1u)] = p;
  else atomicAdd(&pl.rec->finished, 1u);
}

rkh_status bad(const char* who, const std::string& what) {
  set_error(std::string(who) + ": " + what);
  return RKH_ERR_BAD_ARG;
}

enum Phase { PH_SAMPLE, PH_NEAREST, PH_STEER, PH_WALK, PH_COMMIT, PH_COUNT };

}  // namespace
}  // namespace rkh

using namespace rkh;

struct rkh_svp_birrt {
  rkh_scene* scene = nullptr;
  rkh_ctx* ctx = nullptr;
  SvpDev sp;
  uint32_t P = 0;
  DeviceArena arena;
  BiDev d;
  SvpWalk walk;
  std::vector<uint64_t> v_off;  // [P + 1], in rows of both trees
  std::vector<rkh_svp_rrt_params> prm;
  bool failed = false;
  uint32_t live = 0, cur = 0, max_n = 1;
  uint64_t rounds = 0, walk_passes = 0;
  BiRecord rec;
  bool profile = false;
  hipEvent_t ev[PH_COUNT + 1] = {};
  double ms[PH_COUNT] = {};
  ~rkh_svp_birrt() {
    // every entry leaves the stream idle, a failed one perhaps not; the context may be gone already (ctx_give_arena copes)
    if (ctx) (void)hipDeviceSynchronize();
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (arena) ctx_give_arena(ctx, std::move(arena));
  }
};

namespace {

uint32_t blocks_for(uint32_t lanes) { return (lanes + kBiThreads - 1) / kBiThreads; }

// the record after a launch that built live[1 - cur]
rkh_status read_record(rkh_svp_birrt* pl, const char* who, uint32_t next) {
  hipStream_t s = pl->ctx->stream;
  RKH_HIP(hipMemcpyAsync(&pl->rec, pl->d.rec, sizeof(BiRecord), hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  pl->cur = next;
  pl->live = pl->rec.live_cnt[next];
  pl->max_n = std::max(pl->rec.max_n, 1u);
  if (pl->live > pl->P) {
    set_error(std::string(who) + ": the live list is inconsistent");
    return RKH_ERR_DEVICE;
  }
  return RKH_OK;
}

rkh_status one_round(rkh_svp_birrt* pl, const char* who) {
  hipStream_t s = pl->ctx->stream;
  const uint32_t L = pl->live;
  const bool prof = pl->profile;
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_SAMPLE], s));
  hipLaunchKernelGGL(rl1bi_sample_kernel, dim3(L), dim3(kBiThreads), 0, s, pl->sp, pl->d, pl->cur);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_NEAREST], s));
  const uint32_t ns = std::min((pl->max_n + kBiSlice - 1) / kBiSlice, pl->d.slices);
  hipLaunchKernelGGL(rl1bi_nearest_kernel, dim3(ns, L), dim3(kBiThreads), 0, s, pl->sp, pl->d, pl->cur);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_STEER], s));
  hipLaunchKernelGGL(rl1bi_steer_kernel, dim3(blocks_for(L)), dim3(kBiThreads), 0, s, pl->sp, pl->d, pl->walk, pl->cur, L);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_WALK], s));
  uint32_t passes = 0;
  pl->walk.B = L;
  const rkh_status st = launch_svp_walk_dir(who, *pl->scene, pl->sp, pl->walk, pl->d.back, &passes);
  pl->walk_passes += passes;
  RKH_TRY(st);
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_COMMIT], s));
  RKH_HIP(hipMemsetAsync(&pl->d.rec->live_cnt[1 - pl->cur], 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(rl1bi_commit_kernel, dim3(blocks_for(L)), dim3(kBiThreads), 0, s, pl->sp, pl->d, pl->walk, pl->cur, L);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_COUNT], s));
  RKH_TRY(read_record(pl, who, 1 - pl->cur));
  if (prof)
    for (int k = 0; k < PH_COUNT; ++k) {
      float t = 0.0f;
      RKH_HIP(hipEventElapsedTime(&t, pl->ev[k], pl->ev[k + 1]));
      pl->ms[k] += double(t);
    }
  ++pl->rounds;
  return RKH_OK;
}

void fill_stats(const rkh_svp_birrt* pl, rkh_svp_rrt_stats* out) {
  if (!out) return;
  out->rounds = pl->rounds;
  out->problems_finished = pl->rec.finished;
  out->iterations = pl->rec.iterations;
  out->vertices = pl->rec.vertices;
  out->walk_passes = pl->walk_passes;
  out->tested_points = pl->rec.tested;
  out->window_refills = pl->rec.refills;
}

// one tree of a problem, read back whole
struct HostTree {
  std::vector<double> verts, etime;
  std::vector<uint32_t> parent;
};
rkh_status read_tree(const rkh_svp_birrt* pl, const BiProblem& h, uint32_t problem, uint32_t side, HostTree* t) {
  const size_t V = h.n[side], D = 2 * size_t(pl->sp.n), off = size_t(pl->v_off[problem]) + size_t(side) * h.max_vertices;
  t->verts.resize(V * D), t->etime.resize(V), t->parent.resize(V);
  RKH_HIP(hipMemcpy(t->verts.data(), pl->d.verts + off * D, V * D * 8, hipMemcpyDeviceToHost));
  RKH_HIP(hipMemcpy(t->parent.data(), pl->d.parent + off, V * 4, hipMemcpyDeviceToHost));
  RKH_HIP(hipMemcpy(t->etime.data(), pl->d.etime + off, V * 8, hipMemcpyDeviceToHost));
  return RKH_OK;
}

}  // namespace

extern "C" {

rkh_status rkh_svp_birrt_create_batch(rkh_scene* scene, const rkh_svp_space* space, const rkh_svp_rrt_params* params, uint32_t P,
                                      rkh_svp_birrt** out) {
  const char* who = "rkh_svp_birrt_create_batch";
  if (!out) return bad(who, "out is NULL");
  *out = nullptr;
  if (!scene) return bad(who, "scene is NULL");
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, scene->host.n_dof, &sp));
  if (!params) return bad(who, "params is NULL");
  if (P == 0 || P > kBiMaxProblems) return bad(who, "the number of problems must be in [1, 16384]");
  const size_t D = 2 * size_t(sp.n);
  std::vector<uint64_t> v_off(size_t(P) + 1, 0);
  uint32_t largest = 0;
  for (uint32_t i = 0; i < P; ++i) {
    const rkh_svp_rrt_params& pr = params[i];
    const std::string at = "problem " + std::to_string(i) + ": ";
    if (pr.struct_size != sizeof(rkh_svp_rrt_params)) return bad(who, at + "struct_size is not sizeof(rkh_svp_rrt_params)");
    if (pr.max_vertices == 0) return bad(who, at + "max_vertices must be at least 1");
    for (size_t c = 0; c < D; ++c)
      if (!std::isfinite(pr.start[c])) return bad(who, at + "the start is not finite");
    if (!svp_in_bounds(sp, pr.start)) return bad(who, at + "the start is not in bounds (rkh_svp_in_bounds)");
    if (pr.has_goal == 0) return bad(who, at + "has_goal must be 1: a bidirectional problem needs its goal");
    for (size_t c = 0; c < D; ++c)
      if (!std::isfinite(pr.goal[c])) return bad(who, at + "the goal is not finite");
    if (!svp_in_bounds(sp, pr.goal)) return bad(who, at + "the goal is not in bounds (rkh_svp_in_bounds)");
    v_off[i + 1] = v_off[i] + 2 * uint64_t(pr.max_vertices);
    largest = std::max(largest, pr.max_vertices);
  }
  rkh_ctx* ctx = scene->ctx;
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  rkh_svp_birrt* pl = new (std::nothrow) rkh_svp_birrt;
  if (!pl) {
    set_error(std::string(who) + ": out of host memory");
    return RKH_ERR_OOM;
  }
  struct Drop {  // a create that fails leaves no planner behind
    rkh_svp_birrt* p;
    ~Drop() { delete p; }
  } drop{pl};
  pl->scene = scene, pl->sp = sp, pl->P = P;
  pl->v_off = std::move(v_off);
  pl->prm.assign(params, params + P);
  const uint32_t slices = (largest + kBiSlice - 1) / kBiSlice;
  const uint64_t total_v = pl->v_off[P];
  // one slab for the planner: its own ranges, then the walk's workspace for P rows
  size_t cur = 0;
  auto take = [&cur](size_t bytes) {
    ArenaRange r;
    r.off = cur, r.bytes = bytes;
    cur = arena_align_up(cur + bytes);
    return r;
  };
  const ArenaRange r_prob = take(size_t(P) * sizeof(BiProblem)), r_mt = take(size_t(P) * (kRl1MtN + 1) * 4),
                   r_win = take(size_t(P) * kBiWindow * D * 8), r_ok = take(size_t(P) * kBiWindow), r_q = take(size_t(P) * D * 8),
                   r_pd = take(size_t(P) * slices * 8), r_pi = take(size_t(P) * slices * 4), r_v = take(size_t(total_v) * D * 8),
                   r_par = take(size_t(total_v) * 4), r_et = take(size_t(total_v) * 8), r_back = take(size_t(P)),
                   r_l0 = take(size_t(P) * 4), r_l1 = take(size_t(P) * 4), r_rec = take(sizeof(BiRecord));
  const size_t walk_off = cur;
  const size_t bytes = walk_off + svp_walk_layout(sp.n, P, true, nullptr, nullptr) + kArenaGuardBytes;
  RKH_TRY(ctx_take_arena(ctx, bytes, true, &pl->arena));
  pl->ctx = ctx;  // from here the destructor waits for the stream and gives the arena back
  const DeviceArena& A = pl->arena;
  BiDev& d = pl->d;
  d.prob = A.at<BiProblem>(r_prob), d.mt = A.at<uint32_t>(r_mt), d.window = A.at<double>(r_win), d.verdict = A.at<uint8_t>(r_ok);
  d.q = A.at<double>(r_q), d.part_d = A.at<double>(r_pd), d.part_i = A.at<uint32_t>(r_pi), d.verts = A.at<double>(r_v);
  d.parent = A.at<uint32_t>(r_par), d.etime = A.at<double>(r_et), d.back = A.at<uint8_t>(r_back);
  d.live[0] = A.at<uint32_t>(r_l0), d.live[1] = A.at<uint32_t>(r_l1), d.rec = A.at<BiRecord>(r_rec), d.slices = slices;
  svp_walk_layout(sp.n, P, true, static_cast<char*>(A.get()) + walk_off, &pl->walk);
  std::vector<BiProblem> host(P);
  for (uint32_t i = 0; i < P; ++i) {
    const rkh_svp_rrt_params& pr = params[i];
    BiProblem& h = host[i];
    std::memset(&h, 0, sizeof(h));
    h.max_edge_time = pr.max_edge_time, h.steer_tol = pr.steer_tol;
    for (size_t c = 0; c < D; ++c) h.start[c] = pr.start[c], h.goal[c] = pr.goal[c];
    h.v_off = pl->v_off[i];
    h.seed = pr.seed, h.max_vertices = pr.max_vertices, h.max_iterations = pr.max_iterations;
  }
  BiRecord rec0;
  std::memset(&rec0, 0, sizeof(rec0));
  rec0.max_n = 1, rec0.vertices = 2ull * P;
  RKH_HIP(hipMemcpyAsync(d.prob, host.data(), size_t(P) * sizeof(BiProblem), hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemcpyAsync(d.rec, &rec0, sizeof(rec0), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(rl1bi_init_kernel, dim3(P), dim3(kBiThreads), 0, s, sp, d);
  RKH_HIP(hipGetLastError());
  RKH_HIP(hipStreamSynchronize(s));  // host (pageable) is read
  for (hipEvent_t& e : pl->ev) RKH_HIP(hipEventCreate(&e));
  RKH_TRY(read_record(pl, who, 0));
  drop.p = nullptr;
  *out = pl;
  return RKH_OK;
}

void rkh_svp_birrt_destroy(rkh_svp_birrt* planner) { delete planner; }

rkh_status rkh_svp_birrt_solve(rkh_svp_birrt* pl, int64_t max_rounds, rkh_svp_rrt_stats* stats) {
  const char* who = "rkh_svp_birrt_solve";
  if (!pl) return bad(who, "planner is NULL");
  if (pl->failed) {
    set_error(std::string(who) + ": an earlier round of this planner failed");
    return RKH_ERR_DEVICE;
  }
  RKH_HIP(hipSetDevice(pl->ctx->device));
  for (int64_t r = 0; pl->live > 0 && (max_rounds < 0 || r < max_rounds); ++r) {
    const rkh_status st = one_round(pl, who);
    if (st != RKH_OK) {
      pl->failed = true;
      return st;
    }
  }
  fill_stats(pl, stats);
  return RKH_OK;
}

rkh_status rkh_svp_birrt_get_status(rkh_svp_birrt* pl, uint32_t* n_vertices0, uint32_t* n_vertices1, uint32_t* iterations,
                                    uint32_t* join0, uint32_t* join1) {
  const char* who = "rkh_svp_birrt_get_status";
  if (!pl) return bad(who, "planner is NULL");
  RKH_HIP(hipSetDevice(pl->ctx->device));
  std::vector<BiProblem> host(pl->P);
  RKH_HIP(hipMemcpy(host.data(), pl->d.prob, size_t(pl->P) * sizeof(BiProblem), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < pl->P; ++i) {
    if (n_vertices0) n_vertices0[i] = host[i].n[0];
    if (n_vertices1) n_vertices1[i] = host[i].n[1];
    if (iterations) iterations[i] = host[i].iterations;
    if (join0) join0[i] = host[i].join0;
    if (join1) join1[i] = host[i].join1;
  }
  return RKH_OK;
}

rkh_status rkh_svp_birrt_get_tree(rkh_svp_birrt* pl, uint32_t problem, uint32_t tree, double* vertices, uint32_t* parent,
                                  double* edge_time, uint32_t capacity, uint32_t* n_vertices) {
  const char* who = "rkh_svp_birrt_get_tree";
  if (!pl) return bad(who, "planner is NULL");
  if (problem >= pl->P) return bad(who, "no such problem");
  if (tree > 1) return bad(who, "tree must be 0 (from the start) or 1 (from the goal)");
  RKH_HIP(hipSetDevice(pl->ctx->device));
  BiProblem h;
  RKH_HIP(hipMemcpy(&h, pl->d.prob + problem, sizeof(h), hipMemcpyDeviceToHost));
  if (n_vertices) *n_vertices = h.n[tree];
  const size_t V = std::min(h.n[tree], capacity), D = 2 * size_t(pl->sp.n);
  const size_t off = size_t(pl->v_off[problem]) + size_t(tree) * h.max_vertices;
  if (V == 0) return RKH_OK;
  if (vertices) RKH_HIP(hipMemcpy(vertices, pl->d.verts + off * D, V * D * 8, hipMemcpyDeviceToHost));
  if (parent) RKH_HIP(hipMemcpy(parent, pl->d.parent + off, V * 4, hipMemcpyDeviceToHost));
  if (edge_time) RKH_HIP(hipMemcpy(edge_time, pl->d.etime + off, V * 8, hipMemcpyDeviceToHost));
  return RKH_OK;
}

rkh_status rkh_svp_birrt_get_solution(rkh_svp_birrt* pl, uint32_t problem, double* points, uint32_t capacity, uint32_t* n_points,
                                      double* duration) {
  const char* who = "rkh_svp_birrt_get_solution";
  if (!pl) return bad(who, "planner is NULL");
  if (problem >= pl->P) return bad(who, "no such problem");
  if (!n_points) return bad(who, "n_points is NULL");
  *n_points = 0;
  if (duration) *duration = 0.0;
  RKH_HIP(hipSetDevice(pl->ctx->device));
  BiProblem h;
  RKH_HIP(hipMemcpy(&h, pl->d.prob + problem, sizeof(h), hipMemcpyDeviceToHost));
  if (h.join0 == kNone || h.join1 == kNone) return RKH_OK;
  const size_t D = 2 * size_t(pl->sp.n);
  HostTree t0, t1;
  RKH_TRY(read_tree(pl, h, problem, 0, &t0));
  RKH_TRY(read_tree(pl, h, problem, 1, &t1));
  auto chain_of = [who](const HostTree& t, uint32_t from, std::vector<uint32_t>* chain) {
    const size_t V = t.parent.size();
    for (uint32_t v = from; v != kNone; v = t.parent[v]) {
      if (v >= V || chain->size() > V) {
        set_error(std::string(who) + ": the tree is inconsistent");
        return RKH_ERR_DEVICE;
      }
      chain->push_back(v);
    }
    return RKH_OK;
  };
  std::vector<uint32_t> c0, c1;  // c0: join0 ... start, reversed below; c1: join1 ... goal
  RKH_TRY(chain_of(t0, h.join0, &c0));
  RKH_TRY(chain_of(t1, h.join1, &c1));
  std::reverse(c0.begin(), c0.end());
  *n_points = uint32_t(c0.size() + c1.size());
  double sum = 0.0;
  for (size_t k = 1; k < c0.size(); ++k) sum += t0.etime[c0[k]];
  sum += h.join_time;
  for (size_t k = 0; k + 1 < c1.size(); ++k) sum += t1.etime[c1[k]];  // the edge of v runs v -> parent(v); the root has none
  if (duration) *duration = sum;
  if (*n_points > capacity) {
    set_error(std::string(who) + ": the path has more points than capacity");
    return RKH_ERR_CAPACITY;
  }
  if (points) {
    for (size_t k = 0; k < c0.size(); ++k) std::memcpy(points + k * D, t0.verts.data() + size_t(c0[k]) * D, D * 8);
    for (size_t k = 0; k < c1.size(); ++k) std::memcpy(points + (c0.size() + k) * D, t1.verts.data() + size_t(c1[k]) * D, D * 8);
  }
  return RKH_OK;
}

rkh_status rkh_diag_svp_birrt_profile(rkh_svp_birrt* pl, int32_t enable, double* ms) {
  if (!pl) return bad("rkh_diag_svp_birrt_profile", "planner is NULL");
  pl->profile = enable != 0;
  if (ms)
    for (int k = 0; k < PH_COUNT; ++k) ms[k] = pl->ms[k];
  return RKH_OK;
}

}  // extern "C"
