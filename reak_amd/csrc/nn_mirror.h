// nn_mirror.h -- the half-precision MIRROR of a tree that the planner-regime 1-NN sweep reads (nn_mirror.hip).
//
// Beside its fp64 rows [n][Dp] a tree keeps, per vertex, one ready-made A operand of v_mfma_f32_32x32x16_f16: the 16
// k-slots  [ x_h(0) .. x_h(11) | n0 n1 n2 | 0 ].  The mirror lives in PRESCALED units: p = mirror_prescale(coordinate
// bound) is the power of two that brings the bound into [16, 32), x_h(d) = half(float(p x(d))), and a half below the
// normal range (|.| < 2^-14) is stored as 0, so no operand is subnormal and nothing depends on how the matrix
// instruction treats subnormal inputs; |p x - x_h| is MEASURED with the x_h that is stored (nn_mirror.hip, error bound).
// n0, n1, n2 are the float |x_h|^2 split in three halves, each the half nearest to what the pieces before it left, a
// piece below the normal range and those after it 0: n0 + n1 + n2 = |x_h|^2 exactly when all three are normal, and
// within kMirrorSplitLoss = 2^-14 otherwise (rows close to the origin: the threshold's eps carries that term).
// Against a query's B operand  [ -2 q_h(0) .. -2 q_h(11) | 1 1 1 | 0 ]  (q_h from p q in the same way) ONE matrix
// instruction gives c = |x_h|^2 - 2 x_h.q_h = |x_h - q_h|^2 - |q_h|^2 for 32 rows x 32 queries, in units of p^2.
// Without the prescale a half, which resolves 2^-24 at best, cannot hold the squared norms and neighbour distances of a
// small box (side 0.002: |x|^2 ~ 1e-6, d^2 ~ 1e-9), and the sweep returned wrong vertices there.  Rows are stored by
// 32-row slab in the operand's own lane order -- slab s, lane half h, row r: 16 bytes at ((s * 2 + h) * 32 + r) * 16,
// lane (r, h) of a wave loads its fragment with one coalesced 16-byte load, no LDS, no conversion in the sweep -- so
// a sweep reads 32 bytes per vertex where the fp64 rows are 8 Dp.  The mirror is written where rows are written
// (commit_kernel, planner.hip); rows past the end of a tree and removed vertices are PAD rows (coordinates 0, n0 =
// 60000): their estimate is 60000, above every real one, which stays below Dp (2 * 32)^2 = 49152.
//
// The OPEN LISTS of the sweep's second pass, the arithmetic of its work items, the prescale and the threshold of a
// query are stated here once, for the device and for a host compiler (tests/cpp/nn_open_plan_test.cpp and
// tests/cpp/nn_mirror_band_host.cpp read this header without HIP: everything below the threshold is device code and
// only visible to hipcc).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef RKH_HD
#ifdef __HIPCC__
#define RKH_HD __host__ __device__ __forceinline__
#else
#define RKH_HD inline
#endif
#endif

namespace rkh {

// ---- pass 2 of the sweep (nn_mirror.hip): which (row slice, query) pairs it visits, and how a block takes its share
constexpr uint32_t kMirrorGroups = 12;                   // query groups of 32 a block keeps in registers
constexpr uint32_t kMirrorQueries = 32 * kMirrorGroups;  // 384

// Pass 1 leaves est = the smallest estimate of a row slice for a query, the thr kernel the query's threshold thr
// (smallest estimate over all slices + band; +inf for an empty tree).  Pass 2 recomputes the SAME estimates, so a slice
// holds a row with c <= thr iff est <= thr: only then is the query OPEN in the slice.  thr = +inf opens every slice
// (est = +inf included); thr = -inf (a pad slot) opens none; a NaN on either side opens none, as c <= thr records none.
RKH_HD bool mirror_open(float est, float thr) { return est <= thr; }

// Block `block` of a row slice takes the entries [first, first + count) of that slice's query list (of `listed`
// entries: the open list, or the whole batch when the lists are off) as `groups` groups of 32; the last group's `pad`
// slots repeat the block's last entry as an operand and never record (threshold -inf).  count == 0: no work, the block
// leaves.
struct MirrorOpenItem {
  uint32_t first, count, groups, pad;
};
RKH_HD MirrorOpenItem mirror_open_item(uint32_t listed, uint32_t block) {
  MirrorOpenItem it;
  it.first = block * kMirrorQueries;
  it.count = it.first < listed ? (listed - it.first < kMirrorQueries ? listed - it.first : kMirrorQueries) : 0u;
  it.groups = (it.count + 31u) >> 5;
  it.pad = 32u * it.groups - it.count;
  return it;
}
// the list entry slot `slot` (< 32 * groups) of an item reads, and whether the slot may record
RKH_HD uint32_t mirror_open_entry(const MirrorOpenItem& it, uint32_t slot) {
  return it.first + (slot < it.count ? slot : it.count - 1u);
}
RKH_HD bool mirror_open_slot_live(const MirrorOpenItem& it, uint32_t slot) { return slot < it.count; }

// ---- the units of a mirror and the threshold of a query
constexpr double kMirrorMinBound = 1e-3;  // |coordinate| bounds the sweep takes (nn1_mirror_applies)
constexpr double kMirrorMaxBound = 32.0;

// The prescale of a tree: the power of two s with 16 <= s * coord_bound < 32 (host only; the kernels get s as an
// argument).  Scaling by s is exact, so everything the sweep computes is the unscaled problem's times s or s^2.
inline double mirror_prescale(double coord_bound) {
  int e = 0;
  (void)std::frexp(coord_bound, &e);  // coord_bound = m 2^e, 0.5 <= m < 1
  return std::ldexp(1.0, 5 - e);
}

constexpr double kMirrorSplitLoss = 6.103515625e-05;  // 2^-14: what the three pieces of |x_h|^2 may leave out (above)

// The threshold of a query (before it is rounded up to float), in prescaled units: cmin = the smallest estimate over
// the tree, qh2 = |q_h|^2, dq = |q - q_h|, qn = |q|, dx = max |x - x_h| over the rows, X >= |x| for every row.  Rows
// with c <= threshold are a superset of the rows at the true nearest distance (derivation: nn_mirror.hip, error bound).
RKH_HD double mirror_threshold(double cmin, double qh2, double dq, double qn, double dx, double X) {
  const double dxu = dx * (1.0 + 1e-6);
  const double delta = dxu + dq;
  const double Xu = X * (1.0 + 1e-3);  // |x_h| <= |x| (1 + 2^-11)
  const double eps = 1.9073486328125e-06 * (Xu * Xu + 2.0 * Xu * qn) + kMirrorSplitLoss + 1e-9;  // 2^-19 S + ...
  const double base = fmax(0.0, cmin + qh2) + 2.0 * delta * delta + eps;
  const double d_up = delta + sqrt(base) * (1.0 + 1e-12);
  const double E = 2.0 * d_up * delta + delta * delta + eps;
  const double band = 2.0 * E * (1.0 + 1e-9);
  return cmin + band;
}

}  // namespace rkh

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rkh {

constexpr int kMirrorMaxDims = 12;       // coordinates a fragment holds (slots 0..11)
constexpr float kMirrorPadNorm = 60000.0f;

__device__ __forceinline__ uint32_t mirror_half_bits(float v) {  // round to nearest even (v_cvt_f16_f32)
  return uint32_t(__builtin_bit_cast(unsigned short, _Float16(v)));
}
__device__ __forceinline__ float mirror_half_value(uint32_t bits) {
  return float(__builtin_bit_cast(_Float16, (unsigned short)(bits)));
}
// ... and a result below the normal range (exponent field 0) becomes +0: what the operands hold
__device__ __forceinline__ uint32_t mirror_operand_bits(float v) {
  const uint32_t hb = mirror_half_bits(v);
  return (hb & 0x7C00u) ? hb : 0u;
}

// fragment i (16 bytes) of a mirror that holds pad rows only
__device__ __forceinline__ uint4 mirror_pad_fragment(uint64_t i) {
  const bool upper = ((i >> 5) & 1u) != 0u;  // lane half 1 holds slots 8..15: the pad norm sits in slot 12
  return upper ? make_uint4(0u, 0u, mirror_half_bits(kMirrorPadNorm), 0u) : make_uint4(0u, 0u, 0u, 0u);
}

// the two 16-byte fragments (lane half 0: slots 0..7, lane half 1: slots 8..15) of one vertex row, in units of `scale`
// (mirror_prescale); *err = |scale x - x_h| rounded up (0 for a removed vertex)
__device__ __forceinline__ void mirror_row_fragments(const double* __restrict__ row, int D, double scale, uint4* f0, uint4* f1,
                                                     float* err) {
  uint32_t e[16];
  float nrm = 0.0f;
  double e2 = 0.0;
  bool finite = true;
#pragma unroll
  for (int d = 0; d < kMirrorMaxDims; ++d) {
    const double xv = (d < D ? row[d < D ? d : 0] : 0.0) * scale;  // (scaled after the select: the loads stay independent)
    finite = finite && (xv - xv == 0.0);
    const uint32_t hb = mirror_operand_bits(float(xv));
    const float xh = mirror_half_value(hb);
    nrm = __builtin_fmaf(xh, xh, nrm);  // exact products (22 bits), float sum
    e2 += (xv - double(xh)) * (xv - double(xh));
    e[d] = hb;
  }
  *err = finite ? __double2float_ru(sqrt(e2) * (1.0 + 1e-12)) : 0.0f;
  // a piece below the normal range is 0, and so are those after it: what is left out is below 2^-14 (kMirrorSplitLoss)
  const uint32_t n0 = mirror_operand_bits(nrm);
  const float r1 = nrm - mirror_half_value(n0);  // exact
  const uint32_t n1 = n0 ? mirror_operand_bits(r1) : 0u;
  const float r2 = r1 - mirror_half_value(n1);   // exact
  e[12] = n0;
  e[13] = n1;
  e[14] = n1 ? mirror_operand_bits(r2) : 0u;
  e[15] = 0u;
  if (!finite) {  // a removed vertex (+inf row): a pad row
#pragma unroll
    for (int d = 0; d < 16; ++d) e[d] = 0u;
    e[12] = mirror_half_bits(kMirrorPadNorm);
  }
  *f0 = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  *f1 = make_uint4(e[8] | (e[9] << 16), e[10] | (e[11] << 16), e[12] | (e[13] << 16), e[14] | (e[15] << 16));
}

// dx_max_bits: the tree's running maximum of |scale x - x_h| over its rows (bits of a non-negative float: ordered as
// integers)
__device__ __forceinline__ void mirror_store_row(uint4* __restrict__ mirror, uint64_t row, const double* __restrict__ src,
                                                 int D, double scale, uint32_t* __restrict__ dx_max_bits) {
  uint4 f0, f1;
  float err;
  mirror_row_fragments(src, D, scale, &f0, &f1, &err);
  const uint64_t slab = row >> 5, r = row & 31u;
  mirror[(slab * 2 + 0) * 32 + r] = f0;
  mirror[(slab * 2 + 1) * 32 + r] = f1;
  if (err > 0.0f) atomicMax(dx_max_bits, __float_as_uint(err));
}

}  // namespace rkh
#endif  // __HIPCC__
