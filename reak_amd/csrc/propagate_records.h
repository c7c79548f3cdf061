// propagate_records.h -- HIP only: hipcc compiles it into the propagate*.hip units, no host compiler reads it (unlike the
// *_device.h headers).  The bodies of the record kernels (closed forms, support-map forms, depth forms).
#pragma once
#include "propagate_proximity.h"
#include "proximity_record_device.h"

namespace rkh {

// ---- record queries (rkh_min_distance_records, rkh_collision_records) -----------------------------------------------
// One form serves revolute and prismatic chains: proximity_frames with PRISM = true reads SceneDev::prismatic_mask at
// run time and does exactly the revolute arithmetic where the bit is clear, so these kernels exist once, here, and
// rkh::prismatic gains none.  Planar scenes never reach them; scenes with vertex-set shapes reach the *_meshes_kernel forms
// (rkh_min_distance_records_meshes, rkh_collision_records_meshes), whose records of such pairs are gjk_record's.

// Pair pr at the frames proximity_frames left in ws: (shape1, shape2) in the finder's own order, and the gap of their
// bounding spheres (transformToGlobal(0) of both shapes, then |c2 - c1| - r1 - r2: proxy_query_model.cpp:384-389,407-411)
template <typename WS>
RKH_DI double record_pair_shapes(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds, const WS& ws,
                                 const PairDev pr, ShapeG* s1, ShapeG* s2) {
  const ShapeDev& rs = sc->robot[pr.robot];
  const ShapeDev& es = env_lds[pr.env];
  ShapeG A, Bv;
  A.kind = rs.kind;
  A.pos = ld3(ws.Rpos[pr.robot]);
  A.q = ld4(ws.Rquat[pr.robot]);
  A.d0 = rs.dims[0]; A.d1 = rs.dims[1]; A.d2 = rs.dims[2];
  Bv.kind = es.kind;
  Bv.pos = ld3(es.pos);
  Bv.q = ld4(es.quat);
  Bv.d0 = es.dims[0]; Bv.d1 = es.dims[1]; Bv.d2 = es.dims[2];
  *s1 = pr.s1_is_robot ? A : Bv;
  *s2 = pr.s1_is_robot ? Bv : A;
  const d3 c1 = pose_to_parent(s1->pos, s1->q, mk3(0, 0, 0));
  const d3 c2 = pose_to_parent(s2->pos, s2->q, mk3(0, 0, 0));
  const double r1 = pr.s1_is_robot ? rs.brad : es.brad;
  const double r2 = pr.s1_is_robot ? es.brad : rs.brad;
  return norm_2(c2 - c1) - r1 - r2;
}

// The three modes of the record kernels: closed forms only; vertex-set pairs through gjk_distance / gjk_record; the same
// pairs through gjk_depth_distance / gjk_depth_record (a penetration depth where the cores cross, and a normal with
// every record: pair_distance_depth / pair_record_depth).
constexpr int kRecClosed = 0, kRecGjk = 1, kRecDepth = 2;

template <int MODE>
RKH_DI double record_pair_distance(int routine, const ShapeG& s1, const ShapeG& s2, const double* __restrict__ mesh_pool) {
  if constexpr (MODE == kRecDepth) return pair_distance_depth(routine, s1, s2, mesh_pool);
  else return pair_distance<MODE == kRecGjk>(routine, s1, s2, mesh_pool);
}

// slot `at` of the record arrays: the record of pair p (p < 0: no record).  kRecGjk, kRecDepth: vertex-set pairs among
// them, answered from mesh_pool; kRecDepth: three doubles of normal as well (zeros without a record), and the dist of a
// vertex-set pair is its record's own -- gjk_depth_distance's value bit for bit, so a caller need not search twice
template <int MODE = kRecClosed, typename WS>
RKH_DI void write_pair_record(const SceneDev* __restrict__ sc, const ShapeDev* __restrict__ env_lds, const WS& ws,
                              const PairDev* __restrict__ pairs, const PairIdDev* __restrict__ ids, int p, const RecordOut& out,
                              uint64_t at, double dist, const double* __restrict__ mesh_pool = nullptr,
                              double* __restrict__ normal = nullptr) {
  ProxRecordG r;
  r.p1 = r.p2 = mk3(0.0, 0.0, 0.0);
  uint32_t id1 = 0xFFFFFFFFu, id2 = 0xFFFFFFFFu;
  if constexpr (MODE == kRecDepth) {
    d3 nrm = mk3(0.0, 0.0, 0.0);
    if (p >= 0) {
      const PairDev pr = pairs[p];
      ShapeG s1, s2;
      record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
      const ProxRecordN rn = pair_record_depth(pr.routine, s1, s2, mesh_pool);
      r.p1 = rn.p1;
      r.p2 = rn.p2;
      nrm = rn.nrm;
      if (pr.routine == PR_GJK) dist = rn.dist;
      id1 = ids[p].shape1;
      id2 = ids[p].shape2;
    }
    st3(normal + 3 * at, nrm);
  } else if (p >= 0) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    if constexpr (MODE == kRecGjk) r = pair_record<true>(pr.routine, s1, s2, mesh_pool);
    else r = pair_record(pr.routine, s1, s2);
    id1 = ids[p].shape1;
    id2 = ids[p].shape2;
  }
  out.dist[at] = dist;  // the distance the pair was found with (pair_distance), not the point form's own
  st3(out.point1 + 3 * at, r.p1);
  st3(out.point2 + 3 * at, r.p2);
  out.shape1[at] = id1;
  out.shape2[at] = id2;
}

// Kernel: proxy_query_pair_3D::findMinimumDistance()->getLastResult() for B states, one wave per state.  Every lane
// walks its pairs as min_distance_kernel does and keeps two things: the running minimum with that kernel's own
// comparison (so dist is its value bit for bit), and its best (distance, finder rank) in lexicographic order -- the
// reference's loop takes a new minimum only on a strictly smaller distance, so among equal distances the earliest
// finder stays.  A butterfly leaves the wave's winner in every lane; lane 0 evaluates that one pair's point form.
// GJK = true is the form for scenes with vertex-set shapes: it searches with the support-map query as min_distance_kernel
// does there, and lane 0 evaluates the winner's record with gjk_record where the winner is such a pair.  The two forms
// are kernels of their own names (the closed-form one keeps the name and the code it had).  MODE = kRecDepth is the
// third form (min_distance_depth_kernel, in propagate_depth.hip's module): the same search over pair_distance_depth, so
// among crossing vertex-set pairs the deepest wins, and lane 0 writes the winner's normal too.
template <int N, int MODE>
RKH_DI void min_distance_records_body(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                      const PairIdDev* __restrict__ ids, int n_pairs, const double* __restrict__ x, uint32_t B,
                                      const RecordOut& out, double* __restrict__ normal = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const double* mesh_pool = MODE != kRecClosed ? sc->mesh_verts : nullptr;
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  proximity_frames<N, 64, GroupWsQs<N>, true>(sc, sc->robot, cp, lds.base, ws, lds.sink[lane], lane);
  double dmin = INFINITY;
  double dbest = INFINITY;
  uint32_t rbest = 0xFFFFFFFFu;
  int pbest = -1;
  for (int p = lane; p < n_pairs; p += 64) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    const double d = record_pair_distance<MODE>(pr.routine, s1, s2, mesh_pool);
    if (d < dmin) dmin = d;
    const uint32_t rank = ids[p].rank;
    if (d < dbest || (d == dbest && rank < rbest)) {
      dbest = d;
      rbest = rank;
      pbest = p;
    }
  }
  // all lanes are here: the cross-lane reads below run in uniform control flow
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(dmin, off, 64);
    if (o < dmin) dmin = o;
    const double od = __shfl_xor(dbest, off, 64);
    const uint32_t orank = uint32_t(__shfl_xor(int(rbest), off, 64));
    const int op = __shfl_xor(pbest, off, 64);
    if (od < dbest || (od == dbest && orank < rbest)) {
      dbest = od;
      rbest = orank;
      pbest = op;
    }
  }
  if (lane == 0) write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, pbest, out, e, dmin, mesh_pool, normal);
}

// Kernel: proxy_query_pair_3D::gatherCollisionPoints for B states, one wave per state.  Every lane culls and measures
// its pairs (bounding spheres apart: skipped; distance < 0: a collision) and keeps one bit per collision -- pair
// p = 64 s + lane is bit s of (m0, m1), kMaxRecordPairs pairs at most.  The collisions leave in finder order: min(n_found,
// cap) rounds, each a butterfly over every lane's lowest remaining rank; lane 0 evaluates the round's point form and
// the owner drops its bit.  The round count is wave-uniform, so the butterflies run in uniform control flow.
// GJK = true: the form for scenes with vertex-set shapes, as for the minimum-distance records; only lane 0 runs
// gjk_record, between the rounds' butterflies and never around them.  MODE = kRecDepth (collision_depth_kernel): the
// same pairs in the same order (the depth mode keeps the collision mark), their records with depth and normal.
template <int N, int MODE>
RKH_DI void collision_records_body(const SceneDev* __restrict__ sc, const PairDev* __restrict__ pairs,
                                   const PairIdDev* __restrict__ ids, int n_pairs, const double* __restrict__ x, uint32_t B,
                                   uint32_t cap, const RecordOut& out, double* __restrict__ normal = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const double* mesh_pool = MODE != kRecClosed ? sc->mesh_verts : nullptr;
  BlockLdsQs<N, 64>& lds = *reinterpret_cast<BlockLdsQs<N, 64>*>(smem_raw);
  ShapeDev* env_lds = reinterpret_cast<ShapeDev*>(smem_raw + SmemLayoutQs<N, 64>::block_bytes);
  const uint32_t e = blockIdx.x;
  if (e >= B) return;
  const int lane = threadIdx.x;
  constexpr int D = 2 * N;
  stage_chain<N>(sc, lds.joints, lds.base, lane);
  stage_env(sc, env_lds, lane);
  GroupWsQs<N>& ws = lds.g[0];
  if (lane < D) ws.x[lane] = x[uint64_t(e) * D + lane];
  __syncthreads();
  const CPack<N> cp = load_cpack<N>(lds.joints, lane);
  proximity_frames<N, 64, GroupWsQs<N>, true>(sc, sc->robot, cp, lds.base, ws, lds.sink[lane], lane);
  unsigned long long m0 = 0ull, m1 = 0ull;
  for (int p = lane; p < n_pairs; p += 64) {
    const PairDev pr = pairs[p];
    ShapeG s1, s2;
    const double gap = record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
    if (gap > 0.0) continue;
    // (kRecDepth: the depth mode keeps the collision mark, so gjk_distance gives its verdict without the expansion)
    constexpr int VMODE = MODE == kRecDepth ? kRecGjk : MODE;
    if (record_pair_distance<VMODE>(pr.routine, s1, s2, mesh_pool) < 0.0) {
      const int s = p >> 6;
      if (s < 64) m0 |= 1ull << s;
      else m1 |= 1ull << (s - 64);
    }
  }
  uint32_t total = uint32_t(__popcll(m0) + __popcll(m1));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) total += uint32_t(__shfl_xor(int(total), off, 64));
  if (lane == 0) out.n_found[e] = total;
  const uint32_t n_out = total < cap ? total : cap;
  const uint64_t row = uint64_t(e) * cap;
  for (uint32_t k = 0; k < n_out; ++k) {
    uint32_t rmin = 0xFFFFFFFFu;
    int pmin = -1;
    for (unsigned long long mm = m0; mm != 0ull; mm &= mm - 1ull) {
      const int p = ((__ffsll((long long)mm) - 1) << 6) + lane;
      const uint32_t r = ids[p].rank;
      if (r < rmin) rmin = r, pmin = p;
    }
    for (unsigned long long mm = m1; mm != 0ull; mm &= mm - 1ull) {
      const int p = ((__ffsll((long long)mm) - 1 + 64) << 6) + lane;
      const uint32_t r = ids[p].rank;
      if (r < rmin) rmin = r, pmin = p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t orank = uint32_t(__shfl_xor(int(rmin), off, 64));
      const int op = __shfl_xor(pmin, off, 64);
      if (orank < rmin) rmin = orank, pmin = op;
    }
    // (k < total: some lane held a bit, so pmin names a pair)
    if (lane == (pmin & 63)) {
      const int s = pmin >> 6;
      if (s < 64) m0 &= ~(1ull << s);
      else m1 &= ~(1ull << (s - 64));
    }
    if (lane == 0) {
      const PairDev pr = pairs[pmin];
      ShapeG s1, s2;
      record_pair_shapes(sc, env_lds, ws, pr, &s1, &s2);
      // (kRecDepth: a vertex-set pair's dist comes with its record, see write_pair_record)
      constexpr int DMODE = MODE == kRecDepth ? kRecClosed : MODE;
      write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, pmin, out, row + k,
                              record_pair_distance<DMODE>(pr.routine, s1, s2, mesh_pool), mesh_pool, normal);
    }
  }
  for (uint32_t k = n_out + lane; k < cap; k += 64)
    write_pair_record<MODE>(sc, env_lds, ws, pairs, ids, -1, out, row + k, INFINITY, mesh_pool, normal);
}

}  // namespace rkh
