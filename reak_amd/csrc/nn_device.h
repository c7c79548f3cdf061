// nn_device.h -- device code the NN sweeps share (nn_sweep.hip, nn_mirror.hip, knn_sweep.hip; the planner's fix-up).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "rkh_internal.h"

namespace rkh {

typedef float rkh_f16v __attribute__((ext_vector_type(16)));  // accumulator of a 32x32 matrix instruction

// The one dispatch over the padded row widths (nn_padded_dims): f(std::integral_constant<int, DP>()) for the width DP of
// D coordinates -- a padded width maps to itself --; false if D has none.  Host code.
template <class F>
bool with_padded_dims(int D, F&& f) {
  switch (nn_padded_dims(D)) {
    case 2: f(std::integral_constant<int, 2>()); return true;
    case 4: f(std::integral_constant<int, 4>()); return true;
    case 6: f(std::integral_constant<int, 6>()); return true;
    case 8: f(std::integral_constant<int, 8>()); return true;
    case 12: f(std::integral_constant<int, 12>()); return true;
    case 16: f(std::integral_constant<int, 16>()); return true;
    case 24: f(std::integral_constant<int, 24>()); return true;
    case 32: f(std::integral_constant<int, 32>()); return true;
  }
  return false;
}

// The parity contract of every NN form (1-NN and k-NN): the squared distance is the reference's left-to-right sum
//   s = df(0) * df(0),  then  s = s + df(d) * df(d)  for d = 1 .. DP - 1
// over zero-padded coordinates (df(d) = q(d) - x(d); -ffp-contract=off keeps every product and sum rounded), followed
// by the caller's correctly rounded sqrt and lex_less ("first minimum wins").  `diff(d)` reads the operands wherever
// the site keeps them (registers, LDS, the scalar cache, HBM); UNROLL is the unroll count of the loop over d >= 1 (the
// default unrolls it fully).
template <int DP, int UNROLL = DP, class Diff>
__device__ __forceinline__ double nn_exact_sq(const Diff& diff) {
  double s;
  {
    const double df = diff(0);
    s = df * df;
  }
#pragma unroll UNROLL
  for (int d = 1; d < DP; ++d) {
    const double df = diff(d);
    s = s + df * df;
  }
  return s;
}

// coordinate d of a row of D coordinates, zero-padded (coordinate 0 always exists)
__device__ __forceinline__ double nn_qcoord(const double* qq, int d, int D) { return (d == 0 || d < D) ? qq[d] : 0.0; }

// (distance, index) order: ties resolve to the lower vertex index
__device__ __forceinline__ bool lex_less(double da, uint32_t ia, double db, uint32_t ib) {
  return (da < db) || (da == db && ia < ib);
}

// The fields of an NnArgs entry are block-uniform by construction, but they arrive through vector loads: said
// explicitly, they live in scalar registers (scalar row bases, queries through the scalar cache).
__device__ __forceinline__ uint32_t nn_uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t nn_uniform(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v)), hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
  return (uint64_t(hi) << 32) | lo;
}
template <class T>
__device__ __forceinline__ T* nn_uniform(T* p) {
  return reinterpret_cast<T*>(nn_uniform(reinterpret_cast<uint64_t>(p)));
}
__device__ __forceinline__ uint64_t nn_rows(const NnArgs& a) { return nn_uniform(a.d_n ? uint64_t(*a.d_n) : a.n); }
__device__ __forceinline__ uint32_t nn_queries(const NnArgs& a) { return nn_uniform(a.d_B ? *a.d_B : a.B); }
// the first query row of the entry (rows of `stride` coordinates)
__device__ __forceinline__ const double* nn_query_rows(const NnArgs& a, int stride) {
  return nn_uniform(a.q + (a.d_qoff ? uint64_t(*a.d_qoff) : 0ull) * stride);
}

// Work items of the matrix-core sweeps: a 1-D grid of 8 * ceil(W / 8) blocks for W = gx * (query blocks of all
// problems) items (row slice bx, query block by, problem bz).  Hardware deals consecutive blocks round-robin to the 8
// XCDs, so block L runs on XCD L % 8 as that XCD's (L / 8)-th block: XCD x takes the items [x Wc, (x + 1) Wc) in order,
// and items are numbered with the query block fastest -- the query blocks that sweep the same row slice run back to
// back on one XCD and share its L2.  yblock_base: [n_problems + 1] exclusive prefix of the query blocks per problem,
// or nullptr when every problem has gy of them.  False: the block has no item.
__device__ __forceinline__ bool nn_xcd_item(const uint32_t* __restrict__ yblock_base, uint32_t n_problems, uint32_t gx,
                                            uint32_t gy, uint32_t& bx, uint32_t& by, uint32_t& bz) {
  const uint32_t L = blockIdx.x;
  const uint32_t ytot = yblock_base ? yblock_base[n_problems] : gy * n_problems;
  const uint32_t W = ytot * gx, Wc = (W + 7) >> 3;
  const uint32_t slot = L >> 3, w = (L & 7) * Wc + slot;
  if (slot >= Wc || w >= W) return false;
  const uint32_t yy = w / gx;
  uint32_t p = 0, y0, cnt;
  if (yblock_base) {
    uint32_t hi_p = n_problems;  // yblock_base[p] <= yy < yblock_base[hi_p]
    while (hi_p - p > 1) {
      const uint32_t mid = (p + hi_p) >> 1;
      if (yblock_base[mid] <= yy) p = mid;
      else hi_p = mid;
    }
    y0 = yblock_base[p];
    cnt = yblock_base[p + 1] - y0;
  } else {
    p = yy / gy;
    y0 = p * gy;
    cnt = gy;
  }
  const uint32_t r = w - y0 * gx;
  bx = r / cnt;
  by = r - bx * cnt;
  bz = p;
  return true;
}

// The per-lane band-entry list of the matrix-core pre-filters (nn1_sweep_mfma_kernel, nn1_sweep_bf16_kernel,
// nn1_few_mfma_kernel).  A lane holds ONE query and 16 rows of each 32-row slab (the C/D map of the 32x32 shapes:
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  A half slab that holds a row within the band is recorded as ONE
// entry (key, 16-bit row mask, its minimum estimate) in LDS; `rows(key)` is the first row of the entry's half slab, bit
// i of the mask the row rows(key) + 8 (i >> 2) + (i & 3).  When the list is full, the entries the current minimum rules
// out are dropped, and if it is still full the rest is resolved; after the sweep the final minimum cuts it again and
// the survivors are resolved.  `resolve(row)` evaluates a row exactly (nn_exact_sq).
template <int CAP, int THREADS>
struct NnBandLds {
  uint32_t key[CAP][THREADS];
  uint32_t mask[CAP][THREADS];
  float m[CAP][THREADS];
};

template <int CAP, int THREADS, class Rows>
struct NnBandList {
  NnBandLds<CAP, THREADS>& lds;
  const Rows& rows;
  const int tid;
  int cnt;  // entries in the list

  template <class Resolve>
  __device__ __forceinline__ void resolve_entry(int k, const Resolve& resolve) {
    uint32_t mask = lds.mask[k][tid];
    const auto base = rows(lds.key[k][tid]);
#pragma unroll 1
    while (mask) {
      const uint32_t i = uint32_t(__builtin_ctz(mask));
      mask &= mask - 1;
      resolve(base + 8u * (i >> 2) + (i & 3u));
    }
  }
  // drop the entries `lim` rules out; if the list is still full, resolve it
  template <class Resolve>
  __device__ __forceinline__ void compact(float lim, const Resolve& resolve) {
    int w = 0;
#pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
      const float mm = lds.m[k][tid];
      if (mm <= lim) {
        const uint32_t kk = lds.key[k][tid], mk = lds.mask[k][tid];
        lds.m[w][tid] = mm;
        lds.key[w][tid] = kk;
        lds.mask[w][tid] = mk;
        ++w;
      }
    }
    cnt = w;
    if (cnt == CAP) {
#pragma unroll 1
      for (int k = 0; k < cnt; ++k) resolve_entry(k, resolve);
      cnt = 0;
    }
  }
  // the half slab `key` of estimates c, minimum m <= lim
  template <class Resolve>
  __device__ __forceinline__ void record(uint32_t key, const rkh_f16v& c, float m, float lim, const Resolve& resolve) {
    if (cnt == CAP) compact(lim, resolve);
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) mask |= (c[i] <= lim) ? (1u << i) : 0u;
    lds.key[cnt][tid] = key;
    lds.mask[cnt][tid] = mask;
    lds.m[cnt][tid] = m;
    ++cnt;
  }
  // after the sweep: resolve what the final limit leaves of the list
  template <class Resolve>
  __device__ __forceinline__ void finish(float lim, const Resolve& resolve) {
#pragma unroll 1
    for (int k = 0; k < cnt; ++k)
      if (lds.m[k][tid] <= lim) resolve_entry(k, resolve);
  }
};

// the two halves of a wave hold different rows of the same 32 queries: lexicographic minimum over lanes l and l ^ 32
__device__ __forceinline__ void nn_merge_lane_halves(double& best_d, uint32_t& best_i) {
  const double od = __shfl_xor(best_d, 32, 64);
  const uint32_t oi = __shfl_xor(best_i, 32, 64);
  if (lex_less(od, oi, best_d, best_i)) {
    best_d = od;
    best_i = oi;
  }
}

}  // namespace rkh
