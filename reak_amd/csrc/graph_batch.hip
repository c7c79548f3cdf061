// graph_batch.hip -- the kernels and the methods of GraphBatch (graph_batch.h): allocation, command building, the
// launches of one device step and the reference-ordered view of its results.
#include "graph_batch.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rkh {

__global__ void gb_prep_kernel(const GbAux* __restrict__ aux, int DP) {
  const GbAux& a = aux[blockIdx.x];
  if (a.append_dst && int(threadIdx.x) < DP) a.append_dst[threadIdx.x] = threadIdx.x < RKH_MAX_DOF ? a.append_row[threadIdx.x] : 0.0;
}

// first accepted stage-A candidate -> query point of the k-NN and new vertex row (one block of 64 per problem)
__global__ void gb_select_kernel(GbAux* __restrict__ aux, int D, int DP) {
  GbAux& a = aux[blockIdx.x];
  if (a.select_mode == GB_SELECT_NONE) return;
  uint32_t j = 0xFFFFFFFFu;
  for (uint32_t c = 0; c < a.a_count; ++c)
    if (a.a_accept[c]) {
      j = c;
      break;
    }
  if (threadIdx.x == 0) *a.sel = j;
  if (j == 0xFFFFFFFFu) return;
  const int d = threadIdx.x;
  if (d < DP) {
    double v = 0.0;
    if (d < D) v = (a.select_mode == GB_SELECT_POINT) ? a.pts[j][d] : a.a_xout[size_t(j) * D + d];
    if (d < RKH_MAX_DOF) a.query[d] = v;
    a.select_dst[d] = v;
  }
}

// Result blocks -> pinned host memory, written by the device itself, then a step number behind a system-scope fence:
// the host spins on that word instead of sleeping in hipStreamSynchronize (whose wake-up costs more than a whole
// device step of a single planner is worth).  One block per problem; the block that arrives last publishes the step.
__global__ void gb_download_kernel(const uint4* __restrict__ d_res, uint4* __restrict__ h_res, uint32_t words16,
                                   uint32_t* __restrict__ arrivals, volatile uint32_t* __restrict__ h_flag, uint32_t step) {
  const uint4* src = d_res + size_t(blockIdx.x) * words16;
  uint4* dst = h_res + size_t(blockIdx.x) * words16;
  for (uint32_t i = threadIdx.x; i < words16; i += blockDim.x) dst[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(arrivals, 1u) == gridDim.x - 1) {
      *arrivals = 0u;
      __threadfence_system();
      *h_flag = step;
    }
  }
}

__global__ void gb_list_kernel(const GbAux* __restrict__ aux) {
  const GbAux& a = aux[blockIdx.x];
  const bool dropped = (a.select_mode != GB_SELECT_NONE) && (*a.sel == 0xFFFFFFFFu);  // nothing was selected
  const uint32_t K = (a.list_mode == GB_LIST_NONE || dropped) ? 0u : *a.kcnt;
  uint32_t E = 0;
  switch (dropped ? uint32_t(GB_LIST_NONE) : a.list_mode) {
    case GB_LIST_KNN_TO_QUERY:
      E = K;
      for (uint32_t e = threadIdx.x; e < K; e += blockDim.x) a.src_idx[e] = a.kidx[e];
      break;
    case GB_LIST_KNN_BIDIR:
      E = 2 * K;
      for (uint32_t e = threadIdx.x; e < K; e += blockDim.x) {
        a.src_idx[e] = a.kidx[e];
        a.tgt_idx[e] = a.v;
        a.src_idx[K + e] = a.v;
        a.tgt_idx[K + e] = a.kidx[e];
      }
      break;
    case GB_LIST_KNN_TO_VERTEX:
      E = K;
      for (uint32_t e = threadIdx.x; e < K; e += blockDim.x) {
        a.src_idx[e] = a.kidx[e];
        a.tgt_idx[e] = a.v;
      }
      break;
    default: break;
  }
  if (threadIdx.x == 0) *a.n_edges = E;
}

rkh_status GraphBatch::init_dynamic(rkh_scene* sc, const rkh_dyn_space* space, uint32_t n_problems,
                                    const uint64_t* capacities, uint32_t kmax_) {
  if (2 * space->n_dof > RKH_MAX_DOF) {
    set_error("graph batch: state dimension exceeds RKH_MAX_DOF");
    return RKH_ERR_UNSUPPORTED;
  }
  RKH_TRY(build_dyn_dev(*space, 1.0, &dyn));
  dynamic = true;
  steer_req = steer_request();
  std::memset(&qs, 0, sizeof(qs));
  return init_common(sc, 2 * space->n_dof, n_problems, capacities, kmax_);
}

rkh_status GraphBatch::init(rkh_scene* sc, const rkh_qs_space* space, uint32_t n_problems, const uint64_t* capacities,
                            uint32_t kmax_) {
  std::memset(&qs, 0, sizeof(qs));
  qs.min_interval = space->min_interval;
  qs.fraction = 1.0;
  qs_set_speed(qs, space->speed_limits, space->n_dof);
  for (int d = 0; d < space->n_dof; ++d) {
    qs.lower[d] = space->lower[d];
    qs.upper[d] = space->upper[d];
  }
  return init_common(sc, space->n_dof, n_problems, capacities, kmax_);
}

rkh_status GraphBatch::init_common(rkh_scene* sc, int D_, uint32_t n_problems, const uint64_t* capacities,
                                   uint32_t kmax_) {
  scene = sc;
  D = D_;
  DP = nn_padded_dims(D);
  P = n_problems;
  knn_list_cap = knn_list_cap_from_env();
  kmax = kmax_ + 1;  // one neighbour more than asked for: a tie across the k-th place must be visible (neighbours())
  emax = 2 * kmax;
  knn_k.assign(P, 0);
  knn_n.assign(P, 0);
  knn_radius.assign(P, 0.0);
  RKH_HIP(hipSetDevice(sc->ctx->device));
  RKH_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  cmd_bytes = size_t(P) * (sizeof(KnnArgs) + 2 * sizeof(EdgeIO) + sizeof(GbAux));
  RKH_TRY(h_cmd.alloc(cmd_bytes));
  RKH_TRY(d_cmd.alloc(cmd_bytes));
  auto carve = [&](unsigned char* base, KnnArgs** k, EdgeIO** io, EdgeIO** ioa, GbAux** ax) {
    *k = reinterpret_cast<KnnArgs*>(base);
    *io = reinterpret_cast<EdgeIO*>(base + size_t(P) * sizeof(KnnArgs));
    *ioa = reinterpret_cast<EdgeIO*>(base + size_t(P) * (sizeof(KnnArgs) + sizeof(EdgeIO)));
    *ax = reinterpret_cast<GbAux*>(base + size_t(P) * (sizeof(KnnArgs) + 2 * sizeof(EdgeIO)));
  };
  carve(h_cmd.get(), &h_knn, &h_io, &h_ioa, &h_aux);
  carve(d_cmd.get(), &d_knn, &d_io, &d_ioa, &d_aux);
  auto up8 = [](size_t v) { return (v + 7) / 8 * 8; };
  off_kidx = 16;
  off_kdist = up8(off_kidx + size_t(kmax) * 4);
  off_nchk = off_kdist + size_t(kmax) * 8;
  off_accept = off_nchk + size_t(emax) * 4;
  off_xout = up8(off_accept + emax);
  off_anchk = up8(off_xout + size_t(emax) * D * 8);
  off_aaccept = off_anchk + kGbStageA * 4;
  off_axout = up8(off_aaccept + kGbStageA);
  res_stride = (off_axout + size_t(kGbStageA) * D * 8 + 15) / 16 * 16;  // gb_download_kernel moves 16-byte words
  RKH_TRY(h_res.alloc(res_stride * P));
  RKH_TRY(d_res.alloc_zeroed(res_stride * P));
  std::memset(h_res.get(), 0, res_stride * P);
  {  // results written to the host by the device + a flag word the host spins on (gb_download_kernel)
    RKH_TRY(h_flag.alloc(16));  // (a cache line of its own)
    *h_flag.get() = 0u;
    RKH_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_flag_dev), h_flag.get(), 0));
    RKH_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_res_dev), h_res.get(), 0));
    RKH_TRY(d_arrivals.alloc_zeroed(1));
    flag_seq = 0;
  }
  prob.resize(P);
  for (uint32_t i = 0; i < P; ++i) {
    GbProblem& q = prob[i];
    q.tree.D = D;
    q.tree.capacity = (capacities[i] + 255) / 256 * 256;
    RKH_TRY(q.pos.alloc(q.tree.capacity * DP));
    q.tree.d_pos = q.pos.get();
    RKH_TRY(q.d_knn_ws.alloc(kKnnWsBytes));
    RKH_TRY(q.d_src_idx.alloc(emax));
    RKH_TRY(q.d_tgt_idx.alloc(emax));
  }
  begin();
  return RKH_OK;
}

GraphBatch::~GraphBatch() {
  if (!stream) return;
  (void)hipStreamSynchronize(stream);
  (void)hipStreamDestroy(stream);
}

rkh_status GraphBatch::neighbours(uint32_t i, const double* host_pos, const double* query, Neighbours* out,
                                  const uint8_t* removed) {
  const uint32_t kc = kcnt(i), k = knn_k[i];
  const uint32_t* ki = kidx(i);
  const double* kd = kdist(i);
  out->stride = kc;
  out->K = kc < k ? kc : k;
  out->id.assign(ki, ki + out->K);
  out->slot.resize(out->K);
  for (uint32_t e = 0; e < out->K; ++e) out->slot[e] = e;
  bool tie = false;
  for (uint32_t e = 0; e + 1 < kc && e < k; ++e) tie = tie || (kd[e] == kd[e + 1]);
  if (!tie) return RKH_OK;
  // linear k-NN with the reference's heap (the distance is the left-to-right fp64 sum of the device kernels)
  typedef std::pair<double, uint32_t> Entry;
  auto cmp = [](const Entry& a, const Entry& b) { return a.first < b.first; };
  std::vector<Entry> heap;
  double radius = knn_radius[i];
  for (uint64_t v = 0; v < knn_n[i]; ++v) {
    if (removed && removed[v]) continue;  // not a vertex of the graph any more
    double r = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = query[d] - host_pos[v * D + d];
      r += df * df;
    }
    const double dist = std::sqrt(r);
    if (!(dist < radius)) continue;
    heap.push_back(Entry(dist, uint32_t(v)));
    std::push_heap(heap.begin(), heap.end(), cmp);
    if (heap.size() > k) {
      std::pop_heap(heap.begin(), heap.end(), cmp);
      heap.pop_back();
      radius = heap.front().first;
    }
  }
  std::sort_heap(heap.begin(), heap.end(), cmp);
  out->K = uint32_t(heap.size());
  out->id.resize(out->K);
  out->slot.resize(out->K);
  for (uint32_t e = 0; e < out->K; ++e) {
    const uint32_t v = heap[e].second;
    out->id[e] = v;
    uint32_t found = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < kc && found == 0xFFFFFFFFu; ++j)
      if (ki[j] == v) found = j;
    for (uint32_t j = 0; j < kc && found == 0xFFFFFFFFu; ++j)
      if (std::memcmp(&host_pos[size_t(ki[j]) * D], &host_pos[size_t(v) * D], D * sizeof(double)) == 0) found = j;
    if (found == 0xFFFFFFFFu) {
      set_error("graph batch: equal neighbour distances between distinct positions (tie order not reproducible)");
      return RKH_ERR_UNSUPPORTED;
    }
    out->slot[e] = found;
  }
  return RKH_OK;
}

rkh_status GraphBatch::verdicts(uint32_t i, const double* host_pos, const double* query, Verdicts* out,
                                const uint8_t* removed) {
  Neighbours nb;
  rkh_status st = neighbours(i, host_pos, query, &nb, removed);
  if (st != RKH_OK) return st;
  const uint32_t K = nb.K;
  out->K = K;
  out->id = nb.id;
  out->accept.resize(2 * size_t(K));
  out->x_out.resize(2 * size_t(K) * D);
  const uint8_t* acc = accept(i);
  const double* xo = x_out(i);
  for (uint32_t e = 0; e < K; ++e) {
    const uint32_t a = nb.slot[e], b = nb.stride + nb.slot[e];  // b < 2 * kmax = emax: inside the result block
    out->accept[e] = acc[a];
    out->accept[K + e] = acc[b];
    std::memcpy(&out->x_out[size_t(e) * D], &xo[size_t(a) * D], D * sizeof(double));
    std::memcpy(&out->x_out[size_t(K + e) * D], &xo[size_t(b) * D], D * sizeof(double));
  }
  return RKH_OK;
}

void GraphBatch::begin() {
  for (uint32_t i = 0; i < P; ++i) {
    h_knn[i] = KnnArgs();
    h_io[i] = EdgeIO();
    h_ioa[i] = EdgeIO();
    GbAux& a = h_aux[i];
    a.append_dst = nullptr;
    a.a_count = 0;
    a.select_mode = GB_SELECT_NONE;
    a.select_dst = nullptr;
    a.a_accept = dres(i) + off_aaccept;
    a.a_xout = reinterpret_cast<const double*>(dres(i) + off_axout);
    a.sel = reinterpret_cast<uint32_t*>(dres(i)) + 3;
    a.list_mode = GB_LIST_NONE;
    a.v = 0;
    a.kidx = reinterpret_cast<const uint32_t*>(dres(i) + off_kidx);
    a.kcnt = reinterpret_cast<const uint32_t*>(dres(i));
    a.src_idx = prob[i].d_src_idx.get();
    a.tgt_idx = prob[i].d_tgt_idx.get();
    a.n_edges = reinterpret_cast<uint32_t*>(dres(i)) + 2;
  }
  any_knn = any_edges = any_append = any_stage_a = false;
}

rkh_status GraphBatch::cmd_stage_a(uint32_t i, uint32_t select_mode, uint32_t count, uint32_t v, double tol) {
  GbProblem& q = prob[i];
  if (count > kGbStageA || q.n_dev >= q.tree.capacity) {
    set_error("graph batch: stage-A candidate count or vertex capacity exceeded");
    return RKH_ERR_CAPACITY;
  }
  GbAux& a = h_aux[i];
  a.a_count = count;
  a.select_mode = select_mode;
  a.select_dst = q.tree.d_pos + q.n_dev * DP;
  for (uint32_t c = 0; c < kGbStageA; ++c) a.a_src[c] = v;
  EdgeIO& io = h_ioa[i];
  io.src = q.tree.d_pos;
  io.src_idx = d_aux[i].a_src;
  io.src_stride = DP;
  io.tgt = &d_aux[i].pts[0][0];
  io.tgt_stride = RKH_MAX_DOF;
  io.B = count;
  io.x_out = reinterpret_cast<double*>(dres(i) + off_axout);
  io.steps_free = reinterpret_cast<uint32_t*>(dres(i) + off_anchk);
  io.accept = dres(i) + off_aaccept;
  io.err_flag = scene->d_err.get();
  if (select_mode == GB_SELECT_POINT) {
    io.mode = EDGE_POINT;
  } else {
    if (dynamic)  // a walk's travel time is its fraction of the edge time; the kernel's step budget is kMaxSteps
      for (uint32_t c = 0; c < count; ++c)
        if (!(a.frac[c] * dyn.full_time <= kMaxSteps * dyn.dt)) {
          set_error("graph batch: a random walk over the dynamic space asks for more than the step budget of an edge");
          return RKH_ERR_UNSUPPORTED;
        }
    io.mode = EDGE_WALK_ACCEPT;
    io.frac = d_aux[i].frac;
    io.best_case = d_aux[i].target_dist;
    io.steer_tol = tol;
  }
  any_stage_a = true;
  return RKH_OK;
}

rkh_status GraphBatch::remove_row(uint32_t i, uint32_t row) {
  if (inf_row.empty()) inf_row.assign(64, INFINITY);
  GbProblem& q = prob[i];
  if (row >= q.n_dev) {
    set_error("graph batch: no such vertex row");
    return RKH_ERR_BAD_ARG;
  }
  RKH_HIP(hipMemcpyAsync(q.tree.d_pos + uint64_t(row) * DP, inf_row.data(), DP * sizeof(double), hipMemcpyHostToDevice,
                         stream));
  return RKH_OK;
}

rkh_status GraphBatch::cmd_append(uint32_t i, const double* row) {
  GbProblem& q = prob[i];
  if (q.n_dev >= q.tree.capacity || h_aux[i].append_dst) {
    set_error("graph batch: vertex capacity exceeded (or two appends in one step)");
    return RKH_ERR_CAPACITY;
  }
  GbAux& a = h_aux[i];
  for (int d = 0; d < RKH_MAX_DOF; ++d) a.append_row[d] = d < D ? row[d] : 0.0;
  a.append_dst = q.tree.d_pos + q.n_dev * DP;
  ++q.n_dev;
  any_append = true;
  return RKH_OK;
}

rkh_status GraphBatch::cmd_knn(uint32_t i, const double* query, uint64_t n, uint32_t k, double radius) {
  GbProblem& q = prob[i];
  if (k + 1 > kmax) {
    set_error("graph batch: k exceeds the planned maximum");
    return RKH_ERR_CAPACITY;
  }
  knn_k[i] = k;
  knn_n[i] = n;
  knn_radius[i] = radius;
  k += 1;  // see neighbours()
  for (int d = 0; d < RKH_MAX_DOF; ++d) h_aux[i].query[d] = d < D ? query[d] : 0.0;
  KnnArgs& a = h_knn[i];
  size_t bytes = 0;
  rkh_status st = knn_plan_or_error(n, 1, k, &a.ws, &bytes, knn_list_cap);
  if (st != RKH_OK) return st;
  if (bytes > kKnnWsBytes) {
    set_error("graph batch: k-NN workspace too small");
    return RKH_ERR_CAPACITY;
  }
  knn_carve(q.d_knn_ws.get(), 1, &a.ws);
  a.ws.overflow = reinterpret_cast<uint32_t*>(dres(i)) + 1;
  a.pos = q.tree.d_pos;
  a.n = n;
  a.q = d_aux[i].query;
  a.D = D;
  a.B = 1;
  a.k = k;
  a.radius = radius;
  a.m_pow2 = next_pow2(a.ws.m_sub);
  a.out_idx = reinterpret_cast<uint32_t*>(dres(i) + off_kidx);
  a.out_dist = reinterpret_cast<double*>(dres(i) + off_kdist);
  a.out_cnt = reinterpret_cast<uint32_t*>(dres(i));
  any_knn = true;
  return RKH_OK;
}

void GraphBatch::cmd_edges(uint32_t i, uint32_t list_mode, uint32_t v, int mode, double tol) {
  GbProblem& q = prob[i];
  GbAux& a = h_aux[i];
  a.list_mode = list_mode;
  a.v = v;
  EdgeIO& io = h_io[i];
  io.src = q.tree.d_pos;
  io.src_idx = q.d_src_idx.get();
  io.src_stride = DP;
  if (list_mode == GB_LIST_KNN_TO_QUERY) {
    io.tgt = d_aux[i].query;
    io.tgt_stride = 0;
  } else {
    io.tgt = q.tree.d_pos;
    io.tgt_idx = q.d_tgt_idx.get();
    io.tgt_stride = DP;
  }
  io.B = 0;
  io.d_B = reinterpret_cast<const uint32_t*>(dres(i)) + 2;
  io.x_out = reinterpret_cast<double*>(dres(i) + off_xout);
  io.steps_free = reinterpret_cast<uint32_t*>(dres(i) + off_nchk);
  io.accept = dres(i) + off_accept;
  io.mode = mode;
  io.steer_tol = tol;
  io.err_flag = scene->d_err.get();
  any_edges = true;
}

SteerMapping GraphBatch::steer(uint32_t edges) const {
  return steer_mapping(scene->host, SteerEntry::GraphPlanner, steer_req, edges, P, 0);
}

rkh_status GraphBatch::run() {
  hipStream_t s = stream;
  RKH_HIP(hipMemcpyAsync(d_cmd.get(), h_cmd.get(), cmd_bytes, hipMemcpyHostToDevice, s));
  if (any_append) hipLaunchKernelGGL(gb_prep_kernel, dim3(P), dim3(64), 0, s, d_aux, DP);
  if (any_stage_a) {
    rkh_status st = dynamic ? launch_propagate(s, *scene, steer(kGbStageA), dyn, EdgeIO(), kGbStageA, 0, d_ioa, nullptr, P)
                            : launch_edge_check(s, *scene, qs, EdgeIO(), kGbStageA, 0, d_ioa, nullptr, P);
    if (st != RKH_OK) return st;
    hipLaunchKernelGGL(gb_select_kernel, dim3(P), dim3(64), 0, s, d_aux, D, DP);
  }
  if (any_knn) {
    rkh_status st = launch_nnk_table(s, D, d_knn, h_knn, P);
    if (st != RKH_OK) return st;
  }
  RKH_TRY(run_after_knn());
  ++steps;
  if (!knn_overflowed()) return RKH_OK;
  // A problem's first k-NN pass named more vertices than its list holds: the exact retry (knn_plan.h) redoes those
  // problems' searches -- every other problem's neighbourhood is written again as it was -- and what follows the search
  // in a step, a function of the neighbourhoods and of this step's commands alone, runs again on the results.  Rare: a
  // step without an overflow launches nothing of this.
  RKH_TRY(launch_nnk_table_retry(stream, D, d_knn, h_knn, P));
  RKH_TRY(run_after_knn());
  if (knn_overflowed()) {
    set_error(std::string("graph batch: ") + knn_capacity_text());
    return RKH_ERR_CAPACITY;
  }
  return RKH_OK;
}

bool GraphBatch::knn_overflowed() const {
  for (uint32_t i = 0; i < P; ++i)
    if (h_knn[i].B && overflow(i)) return true;
  return false;
}

// the part of a step behind the k-NN search: edge lists, edge walks, and the results' way to the host
rkh_status GraphBatch::run_after_knn() {
  hipStream_t s = stream;
  hipLaunchKernelGGL(gb_list_kernel, dim3(P), dim3(64), 0, s, d_aux);
  if (any_edges) {
    // one wave per edge: a step holds at most 2 k candidates per problem, far from filling the two-lanes mappings
    rkh_status st = dynamic ? launch_propagate(s, *scene, steer(emax), dyn, EdgeIO(), emax, 0, d_io, nullptr, P)
                            : launch_edge_check(s, *scene, qs, EdgeIO(), emax, 0, d_io, nullptr, P);
    if (st != RKH_OK) return st;
  }
  // the results land in pinned host memory; the acquire load of the step word orders the reads of h_res after it
  const uint32_t tag = ++flag_seq;
  hipLaunchKernelGGL(gb_download_kernel, dim3(P), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_res.get()),
                     reinterpret_cast<uint4*>(h_res_dev), uint32_t(res_stride / 16), d_arrivals.get(), h_flag_dev, tag);
  RKH_HIP(hipGetLastError());
  for (uint32_t spins = 0; __atomic_load_n(h_flag.get(), __ATOMIC_ACQUIRE) != tag; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 0xFFFFu) == 0xFFFFu) {  // a failed launch or a device fault must not hang the host
      const hipError_t q = hipStreamQuery(s);
      if (q != hipSuccess && q != hipErrorNotReady) RKH_HIP(q);
      if (q == hipSuccess && __atomic_load_n(h_flag.get(), __ATOMIC_ACQUIRE) != tag) {
        set_error("graph batch: the step's results never arrived");
        return RKH_ERR_DEVICE;
      }
    }
  }
  return RKH_OK;
}

}  // namespace rkh
