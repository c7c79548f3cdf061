// gjk_record_host.cpp -- the record of a support-map (GJK) pair (gjk_record in reak_amd/csrc/gjk_device.h, reached through
// pair_record<true> of proximity_record_device.h) compiled for the host, so that a machine without a GPU can hold its
// points against the exact polytope distance of tests/polytope_ref.py.
//
// Built at test time as a shared library, with the stand-in <hip/hip_runtime.h> of tests/cpp/hip_host first on the path:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I tests/cpp/hip_host -I include tests/cpp/gjk_record_host.cpp
#include "../../reak_amd/csrc/proximity_record_device.h"

namespace {
rkh::ShapeG posed(const rkh_shape& s) {
  rkh::ShapeG g;
  g.kind = s.kind;
  g.pos = rkh::mk3(s.pose.pos[0], s.pose.pos[1], s.pose.pos[2]);
  g.q = rkh::d4{s.pose.quat[0], s.pose.quat[1], s.pose.quat[2], s.pose.quat[3]};
  g.d0 = s.dims[0];
  g.d1 = s.dims[1];
  g.d2 = s.dims[2];
  return g;
}
}  // namespace

extern "C" {

// n pairs of world-anchored shapes (a[i] = shape1) through the PR_GJK routine: [p1 (3), p2 (3), the record's distance,
// gjk_distance of the same build] each
void grh_pair_records(const rkh_shape* a, const rkh_shape* b, int n, const double* pool, double* out) {
  for (int i = 0; i < n; ++i) {
    const rkh::ShapeG s1 = posed(a[i]), s2 = posed(b[i]);
    const rkh::ProxRecordG r = rkh::pair_record<true>(rkh::PR_GJK, s1, s2, pool);
    double* o = out + 8 * i;
    o[0] = r.p1.x; o[1] = r.p1.y; o[2] = r.p1.z;
    o[3] = r.p2.x; o[4] = r.p2.y; o[5] = r.p2.z;
    o[6] = r.dist;
    o[7] = rkh::gjk_distance(rkh::to_gjk(s1, pool), rkh::to_gjk(s2, pool));
  }
}

// pair_record<false> with a pool is the closed-form form: a PR_GJK pair gets no record from it
double grh_no_record(const rkh_shape* a, const rkh_shape* b, const double* pool) {
  return rkh::pair_record<false>(rkh::PR_GJK, posed(*a), posed(*b), pool).dist;
}

}  // extern "C"
