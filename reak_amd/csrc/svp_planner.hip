// svp_planner.hip -- batch RRT over the order-1 rate-limited joint space with SVP profiles (rkh_svp_rrt_*, rkh.h): P
// problems on one scene grow in lock step, one RRT iteration of every unfinished problem per round; trees, sample streams
// and per-problem state live in one arena on the device.  Each problem's tree is the tree of the sequential loop rkh.h
// states (tests/svp_rrt_ref.py), bit for bit: the arithmetic is svp_device.h's, the scalar rules are svp_rrt_device.h's.
//
// A round over the L live problems (the walks are svp_space.hip's staged walk, launch_svp_walk, on device-resident rows):
//   rl1rrt_sample_kernel    one block per live problem: its mt19937 in LDS, regenerated in the three data-parallel
//                           stretches of the recurrence; fills the problem's window of 64 candidates with their bounds
//                           verdicts when the cursor has used it up, takes the next candidate that is in bounds, counts the
//                           skipped ones as iterations and stops at max_iterations -- refills included, no host round trip
//                           (at most 16 refills a launch: a problem that found none sits the round out)
//   rl1rrt_nearest_kernel   one block per (slice of 256 vertices, live problem): every lane solves one whole pair, the
//                           block reduces (time, index) by wave shuffles and one exchange through LDS
//   rl1rrt_steer_kernel     one lane per live problem: merges the slices' minima (ties to the lower index), the steer
//                           fraction, the walk's (a, b, fraction) row
//   [walk: extensions]
//   rl1rrt_commit_kernel    one lane per live problem: the progress rule on d(vertex -> out), appends the vertex with its
//                           parent and edge time, queues the goal probe's row
//   [walk: probes, if any problem has a goal]
//   rl1rrt_finish_kernel    one lane per live problem: goal_parent from the probe, the end conditions, the next round's
//                           live list and the status record the host reads back (one small copy per round)
// Problems without work in a walk (no candidate left, no finite distance, nothing to probe) ride as the row
// (start, start, fraction 0): no point to test, finished by the solve kernel.
#include <cmath>
#include <cstring>
#include <new>

#include "rkh_internal.h"
#include "svp_device.h"
#include "svp_rrt_device.h"

namespace rkh {
namespace {

constexpr uint32_t kRl1Threads = 256;
constexpr uint32_t kRl1Slice = 256;          // vertices per block of the nearest sweep: one pair per lane
constexpr uint32_t kRl1Window = 64;          // candidates generated ahead of a problem's cursor
constexpr uint32_t kRl1RefillsPerLaunch = 16;  // a launch of the sample kernel draws at most 1024 candidates per problem
constexpr uint32_t kRl1MaxProblems = 16384;
constexpr uint32_t kNone = 0xFFFFFFFFu;

enum : uint32_t { kRunning = 0, kGoal = 1, kMaxVertices = 2, kMaxIterations = 3 };
enum : uint32_t { kIdle = 0, kExtend = 1, kAppended = 2 };  // Rl1Problem::step within a round

struct Rl1Problem {  // one problem on the device
  double max_edge_time, steer_tol;
  double start[2 * kSvpMaxDof], goal[2 * kSvpMaxDof];
  uint64_t v_off;  // first row of the problem's tree in the shared vertex arrays
  uint32_t seed, max_vertices, max_iterations, has_goal;
  uint32_t n_vertices, iterations, goal_parent, status;
  uint32_t win_end;  // candidates generated so far: the window holds [win_end - 64, win_end)
  uint32_t refills;
  uint32_t step, nn_idx;
  double asked, fraction;
};

struct Rl1Record {  // what the host reads back after a round
  uint32_t live_cnt[2];
  uint32_t finished, max_n;
  unsigned long long iterations, vertices, tested, refills;
};

struct Rl1Dev {  // device pointers into the planner's arena, by value
  Rl1Problem* prob;    // [P]
  uint32_t* mt;        // [P][624 + 1] generator state + position
  double* window;      // [P][64][2n]
  uint8_t* verdict;    // [P][64]
  double* q;           // [P][2n] the round's candidate
  double* part_d;      // [P][slices]
  uint32_t* part_i;
  double* verts;       // [sum max_vertices][2n]
  uint32_t* parent;    // [sum max_vertices]
  double* etime;
  uint32_t* live[2];   // [P]
  Rl1Record* rec;
  uint32_t slices;     // ceil(largest max_vertices / 256)
};

__device__ __forceinline__ bool rl1_less(double d1, uint32_t i1, double d2, uint32_t i2) {
  return (d1 < d2) || (d1 == d2 && i1 < i2);
}

// the walk row of a problem without work: nothing to solve, nothing to test
__device__ __forceinline__ void rl1_idle_row(const SvpWalk& w, uint32_t l, const double* x, uint32_t D) {
  double* a = const_cast<double*>(w.a) + size_t(l) * D;
  double* b = const_cast<double*>(w.b) + size_t(l) * D;
  for (uint32_t c = 0; c < D; ++c) a[c] = x[c], b[c] = x[c];
  const_cast<double*>(w.fraction)[l] = 0.0;
}

// grid (P).  The arena may have served another planner: whatever a kernel reads before a kernel writes it is written here.
__global__ __launch_bounds__(256) void rl1rrt_init_kernel(const SvpDev sp, const Rl1Dev pl, const SvpWalk w) {
  const uint32_t p = blockIdx.x, tid = threadIdx.x;
  Rl1Problem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  if (tid < D) pl.verts[st.v_off * D + tid] = st.start[tid];
  if (tid < D) {  // the probe before the loop, as a row of the first walk
    const bool probe = st.has_goal != 0;
    const_cast<double*>(w.a)[size_t(p) * D + tid] = st.start[tid];
    const_cast<double*>(w.b)[size_t(p) * D + tid] = probe ? st.goal[tid] : st.start[tid];
    if (tid == 0) const_cast<double*>(w.fraction)[p] = probe ? 1.0 : 0.0;
  }
  if (tid == 64) {
    pl.parent[st.v_off] = kNone;
    pl.etime[st.v_off] = 0.0;
    pl.live[0][p] = p;
    st.n_vertices = 1, st.iterations = 0, st.goal_parent = kNone, st.status = kRunning;
    st.win_end = 0, st.refills = 0, st.nn_idx = 0, st.asked = 0.0, st.fraction = 0.0;
    st.step = st.has_goal ? kAppended : kIdle;
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
__global__ __launch_bounds__(256) void rl1rrt_sample_kernel(const SvpDev sp, const Rl1Dev pl, uint32_t cur) {
  __shared__ uint32_t mt[kRl1MtN];
  __shared__ uint32_t first;
  const uint32_t tid = threadIdx.x;
  const uint32_t p = pl.live[cur][blockIdx.x];
  Rl1Problem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  double* const win = pl.window + size_t(p) * kRl1Window * D;
  uint8_t* const ok = pl.verdict + size_t(p) * kRl1Window;
  uint32_t* const g_mt = pl.mt + size_t(p) * (kRl1MtN + 1);
  const uint32_t it0 = st.iterations, max_it = st.max_iterations;
  uint32_t it = it0, win_end = st.win_end;
  uint32_t found = kNone, refills = 0, idx = 0;
  bool loaded = false;
  __syncthreads();  // everybody has read the state lane 0 writes at the end
  while (true) {  // uniform
    if (it == win_end) {
      if (!loaded) {
        for (uint32_t i = tid; i < kRl1MtN; i += kRl1Threads) mt[i] = g_mt[i];
        idx = g_mt[kRl1MtN];
        loaded = true;
        __syncthreads();
      }
      const uint32_t count = kRl1Window * D;
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
          stretch(0, kRl1MtN - kRl1MtM);                      // 0 .. 226
          stretch(kRl1MtN - kRl1MtM, 2 * (kRl1MtN - kRl1MtM));  // 227 .. 453
          stretch(2 * (kRl1MtN - kRl1MtM), kRl1MtN - 1);      // 454 .. 622
          if (tid == 0) mt[kRl1MtN - 1] = rl1rrt_mt_twist(mt[kRl1MtN - 1], mt[0], mt[kRl1MtM - 1]);
          __syncthreads();
          idx = 0;
        }
        const uint32_t left = count - produced;
        const uint32_t chunk = (kRl1MtN - idx < left) ? kRl1MtN - idx : left;
        for (uint32_t t = tid; t < chunk; t += kRl1Threads) {
          const double u = rl1rrt_unit(rl1rrt_mt_temper(mt[idx + t]));
          double lo, hi;
          rl1rrt_coord_range(sp, (produced + t) % D, &lo, &hi);
          win[produced + t] = rl1rrt_coord(lo, hi, u);
        }
        produced += chunk;
        idx += chunk;
        __syncthreads();
      }
      if (tid < kRl1Window) ok[tid] = svp_in_bounds(sp, win + size_t(tid) * D) ? 1 : 0;
      __syncthreads();
      win_end += kRl1Window;
      ++refills;
    }
    const uint32_t avail = win_end - it, left_it = max_it - it;
    const uint32_t lim = avail < left_it ? avail : left_it;  // 1 .. 64
    const uint32_t slot0 = kRl1Window - avail;
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
    // a box that rejects (nearly) everything: the problem sits this round out and draws on in the next, so that no
    // launch runs for max_iterations candidates
    if (refills >= kRl1RefillsPerLaunch) break;
  }
  if (loaded) {
    for (uint32_t i = tid; i < kRl1MtN; i += kRl1Threads) g_mt[i] = mt[i];
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
__global__ __launch_bounds__(256) void rl1rrt_nearest_kernel(const SvpDev sp, const Rl1Dev pl, uint32_t cur) {
  __shared__ double qv[2 * kSvpMaxDof];
  __shared__ double red_d[kRl1Threads / 64];
  __shared__ uint32_t red_i[kRl1Threads / 64];
  const uint32_t tid = threadIdx.x, s = blockIdx.x;
  const uint32_t p = pl.live[cur][blockIdx.y];
  const Rl1Problem& st = pl.prob[p];
  const uint32_t n = st.n_vertices, base = s * kRl1Slice;
  if (st.step != kExtend || base >= n) return;  // uniform
  const uint32_t D = 2 * uint32_t(sp.n);
  if (tid < D) qv[tid] = pl.q[size_t(p) * D + tid];
  __syncthreads();
  const uint32_t g = base + tid;
  double d = INFINITY;
  uint32_t i = kNone;
  if (g < n) {
    d = svp_reach(sp, pl.verts + (st.v_off + g) * D, qv, nullptr);
    i = g;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const double od = __shfl_xor(d, m, 64);
    const uint32_t oi = __shfl_xor(i, m, 64);
    if (rl1_less(od, oi, d, i)) d = od, i = oi;
  }
  if ((tid & 63) == 0) red_d[tid >> 6] = d, red_i[tid >> 6] = i;
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < kRl1Threads / 64; ++w)
      if (rl1_less(red_d[w], red_i[w], d, i)) d = red_d[w], i = red_i[w];
    pl.part_d[size_t(p) * pl.slices + s] = d;
    pl.part_i[size_t(p) * pl.slices + s] = i;
  }
}

// one lane per live problem
__global__ __launch_bounds__(256) void rl1rrt_steer_kernel(const SvpDev sp, const Rl1Dev pl, const SvpWalk w, uint32_t cur,
                                                           uint32_t L) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint32_t p = pl.live[cur][l];
  Rl1Problem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  double d = INFINITY;
  uint32_t i = kNone;
  if (st.step == kExtend) {
    const uint32_t ns = (st.n_vertices + kRl1Slice - 1) / kRl1Slice;
    for (uint32_t s = 0; s < ns; ++s) {  // ascending slices hold ascending indices: "less" keeps the lower one of a tie
      const double sd = pl.part_d[size_t(p) * pl.slices + s];
      if (sd < d) d = sd, i = pl.part_i[size_t(p) * pl.slices + s];
    }
  }
  if (!(d < INFINITY)) {
    st.step = kIdle;
    rl1_idle_row(w, l, st.start, D);
    return;
  }
  const double f = rl1rrt_fraction(d, st.max_edge_time);
  st.nn_idx = i, st.asked = d, st.fraction = f;
  const double* v = pl.verts + (st.v_off + i) * D;
  const double* q = pl.q + size_t(p) * D;
  double* a = const_cast<double*>(w.a) + size_t(l) * D;
  double* b = const_cast<double*>(w.b) + size_t(l) * D;
  for (uint32_t c = 0; c < D; ++c) a[c] = v[c], b[c] = q[c];
  const_cast<double*>(w.fraction)[l] = f;
}

// one lane per live problem, after the extensions' walk
__global__ __launch_bounds__(256) void rl1rrt_commit_kernel(const SvpDev sp, const Rl1Dev pl, const SvpWalk w, uint32_t cur,
                                                            uint32_t L) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint32_t p = pl.live[cur][l];
  Rl1Problem& st = pl.prob[p];
  const uint32_t D = 2 * uint32_t(sp.n);
  double* a = const_cast<double*>(w.a) + size_t(l) * D;
  double* b = const_cast<double*>(w.b) + size_t(l) * D;
  const double* out = w.out + size_t(l) * D;
  uint32_t step = kIdle;
  if (st.step == kExtend) {
    const uint32_t nc = w.n_checked[l];
    if (nc) {
      atomicAdd(&pl.rec->tested, (unsigned long long)nc);
      const double travelled = svp_reach(sp, a, out, nullptr);
      if (rl1rrt_progress(travelled, st.asked, st.fraction, st.steer_tol)) {
        const uint32_t v = st.n_vertices;
        double* row = pl.verts + (st.v_off + v) * D;
        for (uint32_t c = 0; c < D; ++c) row[c] = out[c];
        pl.parent[st.v_off + v] = st.nn_idx;
        pl.etime[st.v_off + v] = travelled;
        st.n_vertices = v + 1;
        atomicAdd(&pl.rec->vertices, 1ull);
        atomicMax(&pl.rec->max_n, v + 1);
        step = kAppended;
      }
    }
  }
  st.step = step;
  if (step == kAppended && st.has_goal) {
    for (uint32_t c = 0; c < D; ++c) a[c] = out[c], b[c] = st.goal[c];
    const_cast<double*>(w.fraction)[l] = 1.0;
  } else {
    rl1_idle_row(w, l, st.start, D);
  }
}

// one lane per live problem, after the probes' walk (probed = 0: no problem of the batch has a goal, no walk ran)
__global__ __launch_bounds__(256) void rl1rrt_finish_kernel(const Rl1Dev pl, const SvpWalk w, uint32_t cur, uint32_t L,
                                                            int probed) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= L) return;
  const uint32_t p = pl.live[cur][l];
  Rl1Problem& st = pl.prob[p];
  if (probed && st.step == kAppended && st.has_goal) {
    const uint32_t nc = w.n_checked[l];
    if (nc) atomicAdd(&pl.rec->tested, (unsigned long long)nc);
    if (w.reached[l]) st.goal_parent = st.n_vertices - 1;
  }
  st.step = kIdle;
  uint32_t status = kRunning;
  if (st.goal_parent != kNone) status = kGoal;
  else if (st.n_vertices >= st.max_vertices) status = kMaxVertices;
  else if (st.iterations >= st.max_iterations) status = kMaxIterations;
  st.status = status;
  if (status == kRunning) pl.live[1 - cur][atomicAdd(&pl.rec->live_cnt[1 - cur], 1u)] = p;
  else atomicAdd(&pl.rec->finished, 1u);
}

rkh_status bad(const char* who, const std::string& what) {
  set_error(std::string(who) + ": " + what);
  return RKH_ERR_BAD_ARG;
}

enum Phase { PH_SAMPLE, PH_NEAREST, PH_EXTEND, PH_COMMIT, PH_PROBE, PH_FINISH, PH_COUNT };

}  // namespace
}  // namespace rkh

using namespace rkh;

struct rkh_svp_rrt {
  rkh_scene* scene = nullptr;
  rkh_ctx* ctx = nullptr;
  SvpDev sp;
  uint32_t P = 0;
  DeviceArena arena;
  Rl1Dev d;
  SvpWalk walk;
  std::vector<uint64_t> v_off;  // [P + 1]
  std::vector<rkh_svp_rrt_params> prm;
  bool any_goal = false, failed = false;
  uint32_t live = 0, cur = 0, max_n = 1;
  uint64_t rounds = 0, walk_passes = 0;
  Rl1Record rec;
  bool profile = false;
  hipEvent_t ev[PH_COUNT + 1] = {};
  double ms[PH_COUNT] = {};
  ~rkh_svp_rrt() {
    // every entry leaves the stream idle, a failed one perhaps not; the context may be gone already (ctx_give_arena copes)
    if (ctx) (void)hipDeviceSynchronize();
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (arena) ctx_give_arena(ctx, std::move(arena));
  }
};

namespace {

uint32_t blocks_for(uint32_t lanes) { return (lanes + kRl1Threads - 1) / kRl1Threads; }

// the probes' walk and the finish pass over the L problems of live[cur]; reads the record back
rkh_status finish_round(rkh_svp_rrt* pl, const char* who, uint32_t L) {
  hipStream_t s = pl->ctx->stream;
  if (pl->any_goal) {
    uint32_t passes = 0;
    pl->walk.B = L;
    const rkh_status st = launch_svp_walk(who, *pl->scene, pl->sp, pl->walk, &passes);
    pl->walk_passes += passes;
    RKH_TRY(st);
  }
  if (pl->profile) RKH_HIP(hipEventRecord(pl->ev[PH_FINISH], s));
  RKH_HIP(hipMemsetAsync(&pl->d.rec->live_cnt[1 - pl->cur], 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(rl1rrt_finish_kernel, dim3(blocks_for(L)), dim3(kRl1Threads), 0, s, pl->d, pl->walk, pl->cur, L,
                     pl->any_goal ? 1 : 0);
  RKH_HIP(hipGetLastError());
  if (pl->profile) RKH_HIP(hipEventRecord(pl->ev[PH_COUNT], s));
  RKH_HIP(hipMemcpyAsync(&pl->rec, pl->d.rec, sizeof(Rl1Record), hipMemcpyDeviceToHost, s));
  RKH_HIP(hipStreamSynchronize(s));
  pl->cur = 1 - pl->cur;
  pl->live = pl->rec.live_cnt[pl->cur];
  pl->max_n = std::max(pl->rec.max_n, 1u);
  if (pl->live > pl->P) {
    set_error(std::string(who) + ": the live list is inconsistent");
    return RKH_ERR_DEVICE;
  }
  return RKH_OK;
}

rkh_status one_round(rkh_svp_rrt* pl, const char* who) {
  hipStream_t s = pl->ctx->stream;
  const uint32_t L = pl->live;
  const bool prof = pl->profile;
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_SAMPLE], s));
  hipLaunchKernelGGL(rl1rrt_sample_kernel, dim3(L), dim3(kRl1Threads), 0, s, pl->sp, pl->d, pl->cur);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_NEAREST], s));
  const uint32_t ns = std::min((pl->max_n + kRl1Slice - 1) / kRl1Slice, pl->d.slices);
  hipLaunchKernelGGL(rl1rrt_nearest_kernel, dim3(ns, L), dim3(kRl1Threads), 0, s, pl->sp, pl->d, pl->cur);
  RKH_HIP(hipGetLastError());
  hipLaunchKernelGGL(rl1rrt_steer_kernel, dim3(blocks_for(L)), dim3(kRl1Threads), 0, s, pl->sp, pl->d, pl->walk, pl->cur, L);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_EXTEND], s));
  uint32_t passes = 0;
  pl->walk.B = L;
  const rkh_status st = launch_svp_walk(who, *pl->scene, pl->sp, pl->walk, &passes);
  pl->walk_passes += passes;
  RKH_TRY(st);
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_COMMIT], s));
  hipLaunchKernelGGL(rl1rrt_commit_kernel, dim3(blocks_for(L)), dim3(kRl1Threads), 0, s, pl->sp, pl->d, pl->walk, pl->cur, L);
  RKH_HIP(hipGetLastError());
  if (prof) RKH_HIP(hipEventRecord(pl->ev[PH_PROBE], s));
  RKH_TRY(finish_round(pl, who, L));
  if (prof)
    for (int k = 0; k < PH_COUNT; ++k) {
      float t = 0.0f;
      RKH_HIP(hipEventElapsedTime(&t, pl->ev[k], pl->ev[k + 1]));
      pl->ms[k] += double(t);
    }
  ++pl->rounds;
  return RKH_OK;
}

void fill_stats(const rkh_svp_rrt* pl, rkh_svp_rrt_stats* out) {
  if (!out) return;
  out->rounds = pl->rounds;
  out->problems_finished = pl->rec.finished;
  out->iterations = pl->rec.iterations;
  out->vertices = pl->rec.vertices;
  out->walk_passes = pl->walk_passes;
  out->tested_points = pl->rec.tested;
  out->window_refills = pl->rec.refills;
}

}  // namespace

extern "C" {

rkh_status rkh_svp_rrt_create_batch(rkh_scene* scene, const rkh_svp_space* space, const rkh_svp_rrt_params* params, uint32_t P,
                                    rkh_svp_rrt** out) {
  const char* who = "rkh_svp_rrt_create_batch";
  if (!out) return bad(who, "out is NULL");
  *out = nullptr;
  if (!scene) return bad(who, "scene is NULL");
  SvpDev sp;
  RKH_TRY(svp_space_dev(who, space, scene->host.n_dof, &sp));
  if (!params) return bad(who, "params is NULL");
  if (P == 0 || P > kRl1MaxProblems) return bad(who, "the number of problems must be in [1, 16384]");
  const size_t D = 2 * size_t(sp.n);
  std::vector<uint64_t> v_off(size_t(P) + 1, 0);
  uint32_t largest = 0;
  bool any_goal = false;
  for (uint32_t i = 0; i < P; ++i) {
    const rkh_svp_rrt_params& pr = params[i];
    const std::string at = "problem " + std::to_string(i) + ": ";
    if (pr.struct_size != sizeof(rkh_svp_rrt_params)) return bad(who, at + "struct_size is not sizeof(rkh_svp_rrt_params)");
    if (pr.max_vertices == 0) return bad(who, at + "max_vertices must be at least 1");
    for (size_t c = 0; c < D; ++c)
      if (!std::isfinite(pr.start[c])) return bad(who, at + "the start is not finite");
    if (!svp_in_bounds(sp, pr.start)) return bad(who, at + "the start is not in bounds (rkh_svp_in_bounds)");
    v_off[i + 1] = v_off[i] + pr.max_vertices;
    largest = std::max(largest, pr.max_vertices);
    any_goal = any_goal || pr.has_goal != 0;
  }
  rkh_ctx* ctx = scene->ctx;
  hipStream_t s = ctx->stream;
  RKH_HIP(hipSetDevice(ctx->device));
  rkh_svp_rrt* pl = new (std::nothrow) rkh_svp_rrt;
  if (!pl) {
    set_error(std::string(who) + ": out of host memory");
    return RKH_ERR_OOM;
  }
  struct Drop {  // a create that fails leaves no planner behind
    rkh_svp_rrt* p;
    ~Drop() { delete p; }
  } drop{pl};
  pl->scene = scene, pl->sp = sp, pl->P = P, pl->any_goal = any_goal;
  pl->v_off = std::move(v_off);
  pl->prm.assign(params, params + P);
  const uint32_t slices = (largest + kRl1Slice - 1) / kRl1Slice;
  const uint64_t total_v = pl->v_off[P];
  // one slab for the planner: its own ranges, then the walk's workspace for P edges
  size_t cur = 0;
  auto take = [&cur](size_t bytes) {
    ArenaRange r;
    r.off = cur, r.bytes = bytes;
    cur = arena_align_up(cur + bytes);
    return r;
  };
  const ArenaRange r_prob = take(size_t(P) * sizeof(Rl1Problem)), r_mt = take(size_t(P) * (kRl1MtN + 1) * 4),
                   r_win = take(size_t(P) * kRl1Window * D * 8), r_ok = take(size_t(P) * kRl1Window), r_q = take(size_t(P) * D * 8),
                   r_pd = take(size_t(P) * slices * 8), r_pi = take(size_t(P) * slices * 4), r_v = take(size_t(total_v) * D * 8),
                   r_par = take(size_t(total_v) * 4), r_et = take(size_t(total_v) * 8), r_l0 = take(size_t(P) * 4),
                   r_l1 = take(size_t(P) * 4), r_rec = take(sizeof(Rl1Record));
  const size_t walk_off = cur;
  const size_t bytes = walk_off + svp_walk_layout(sp.n, P, true, nullptr, nullptr) + kArenaGuardBytes;
  RKH_TRY(ctx_take_arena(ctx, bytes, true, &pl->arena));
  pl->ctx = ctx;  // from here the destructor waits for the stream and gives the arena back
  const DeviceArena& A = pl->arena;
  Rl1Dev& d = pl->d;
  d.prob = A.at<Rl1Problem>(r_prob), d.mt = A.at<uint32_t>(r_mt), d.window = A.at<double>(r_win), d.verdict = A.at<uint8_t>(r_ok);
  d.q = A.at<double>(r_q), d.part_d = A.at<double>(r_pd), d.part_i = A.at<uint32_t>(r_pi), d.verts = A.at<double>(r_v);
  d.parent = A.at<uint32_t>(r_par), d.etime = A.at<double>(r_et), d.live[0] = A.at<uint32_t>(r_l0), d.live[1] = A.at<uint32_t>(r_l1);
  d.rec = A.at<Rl1Record>(r_rec), d.slices = slices;
  svp_walk_layout(sp.n, P, true, static_cast<char*>(A.get()) + walk_off, &pl->walk);
  std::vector<Rl1Problem> host(P);
  for (uint32_t i = 0; i < P; ++i) {
    const rkh_svp_rrt_params& pr = params[i];
    Rl1Problem& h = host[i];
    std::memset(&h, 0, sizeof(h));
    h.max_edge_time = pr.max_edge_time, h.steer_tol = pr.steer_tol;
    for (size_t c = 0; c < D; ++c) h.start[c] = pr.start[c], h.goal[c] = pr.has_goal ? pr.goal[c] : pr.start[c];
    h.v_off = pl->v_off[i];
    h.seed = pr.seed, h.max_vertices = pr.max_vertices, h.max_iterations = pr.max_iterations, h.has_goal = pr.has_goal ? 1u : 0u;
  }
  Rl1Record rec0;
  std::memset(&rec0, 0, sizeof(rec0));
  rec0.max_n = 1, rec0.vertices = P;
  RKH_HIP(hipMemcpyAsync(d.prob, host.data(), size_t(P) * sizeof(Rl1Problem), hipMemcpyHostToDevice, s));
  RKH_HIP(hipMemcpyAsync(d.rec, &rec0, sizeof(rec0), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(rl1rrt_init_kernel, dim3(P), dim3(kRl1Threads), 0, s, sp, d, pl->walk);
  RKH_HIP(hipGetLastError());
  RKH_HIP(hipStreamSynchronize(s));  // host (pageable) is read
  for (hipEvent_t& e : pl->ev) RKH_HIP(hipEventCreate(&e));
  // the probes before the loop, and the problems that have ended before their first iteration
  pl->cur = 0, pl->live = P;
  RKH_TRY(finish_round(pl, who, P));
  drop.p = nullptr;
  *out = pl;
  return RKH_OK;
}

void rkh_svp_rrt_destroy(rkh_svp_rrt* planner) { delete planner; }

rkh_status rkh_svp_rrt_solve(rkh_svp_rrt* pl, int64_t max_rounds, rkh_svp_rrt_stats* stats) {
  const char* who = "rkh_svp_rrt_solve";
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

rkh_status rkh_svp_rrt_get_status(rkh_svp_rrt* pl, uint32_t* n_vertices, uint32_t* iterations, uint32_t* goal_parent) {
  const char* who = "rkh_svp_rrt_get_status";
  if (!pl) return bad(who, "planner is NULL");
  RKH_HIP(hipSetDevice(pl->ctx->device));
  std::vector<Rl1Problem> host(pl->P);
  RKH_HIP(hipMemcpy(host.data(), pl->d.prob, size_t(pl->P) * sizeof(Rl1Problem), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < pl->P; ++i) {
    if (n_vertices) n_vertices[i] = host[i].n_vertices;
    if (iterations) iterations[i] = host[i].iterations;
    if (goal_parent) goal_parent[i] = host[i].goal_parent;
  }
  return RKH_OK;
}

rkh_status rkh_svp_rrt_get_tree(rkh_svp_rrt* pl, uint32_t problem, double* vertices, uint32_t* parent, double* edge_time,
                                uint32_t capacity, uint32_t* n_vertices) {
  const char* who = "rkh_svp_rrt_get_tree";
  if (!pl) return bad(who, "planner is NULL");
  if (problem >= pl->P) return bad(who, "no such problem");
  RKH_HIP(hipSetDevice(pl->ctx->device));
  Rl1Problem h;
  RKH_HIP(hipMemcpy(&h, pl->d.prob + problem, sizeof(h), hipMemcpyDeviceToHost));
  if (n_vertices) *n_vertices = h.n_vertices;
  const size_t V = std::min(h.n_vertices, capacity), D = 2 * size_t(pl->sp.n), off = size_t(pl->v_off[problem]);
  if (V == 0) return RKH_OK;
  if (vertices) RKH_HIP(hipMemcpy(vertices, pl->d.verts + off * D, V * D * 8, hipMemcpyDeviceToHost));
  if (parent) RKH_HIP(hipMemcpy(parent, pl->d.parent + off, V * 4, hipMemcpyDeviceToHost));
  if (edge_time) RKH_HIP(hipMemcpy(edge_time, pl->d.etime + off, V * 8, hipMemcpyDeviceToHost));
  return RKH_OK;
}

rkh_status rkh_svp_rrt_get_solution(rkh_svp_rrt* pl, uint32_t problem, double* points, uint32_t capacity, uint32_t* n_points,
                                    double* duration) {
  const char* who = "rkh_svp_rrt_get_solution";
  if (!pl) return bad(who, "planner is NULL");
  if (problem >= pl->P) return bad(who, "no such problem");
  if (!n_points) return bad(who, "n_points is NULL");
  *n_points = 0;
  if (duration) *duration = 0.0;
  RKH_HIP(hipSetDevice(pl->ctx->device));
  Rl1Problem h;
  RKH_HIP(hipMemcpy(&h, pl->d.prob + problem, sizeof(h), hipMemcpyDeviceToHost));
  if (h.goal_parent == kNone) return RKH_OK;
  const size_t V = h.n_vertices, D = 2 * size_t(pl->sp.n), off = size_t(pl->v_off[problem]);
  std::vector<double> verts(V * D), etime(V);
  std::vector<uint32_t> parent(V);
  RKH_HIP(hipMemcpy(verts.data(), pl->d.verts + off * D, V * D * 8, hipMemcpyDeviceToHost));
  RKH_HIP(hipMemcpy(parent.data(), pl->d.parent + off, V * 4, hipMemcpyDeviceToHost));
  RKH_HIP(hipMemcpy(etime.data(), pl->d.etime + off, V * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> chain;
  for (uint32_t v = h.goal_parent; v != kNone; v = parent[v]) {
    if (v >= V || chain.size() > V) {
      set_error(std::string(who) + ": the tree is inconsistent");
      return RKH_ERR_DEVICE;
    }
    chain.push_back(v);
  }
  std::reverse(chain.begin(), chain.end());
  *n_points = uint32_t(chain.size() + 1);
  double sum = 0.0;
  for (size_t k = 1; k < chain.size(); ++k) sum += etime[chain[k]];
  sum += svp_reach(pl->sp, verts.data() + size_t(chain.back()) * D, h.goal, nullptr);
  if (duration) *duration = sum;
  if (*n_points > capacity) {
    set_error(std::string(who) + ": the path has more points than capacity");
    return RKH_ERR_CAPACITY;
  }
  if (points) {
    for (size_t k = 0; k < chain.size(); ++k) std::memcpy(points + k * D, verts.data() + size_t(chain[k]) * D, D * 8);
    std::memcpy(points + chain.size() * D, h.goal, D * 8);
  }
  return RKH_OK;
}

rkh_status rkh_diag_svp_rrt_profile(rkh_svp_rrt* pl, int32_t enable, double* ms) {
  if (!pl) return bad("rkh_diag_svp_rrt_profile", "planner is NULL");
  pl->profile = enable != 0;
  if (ms)
    for (int k = 0; k < PH_COUNT; ++k) ms[k] = pl->ms[k];
  return RKH_OK;
}

}  // extern "C"
