// prox_record_host.cpp -- the device's closed forms with points (reak_amd/csrc/proximity_record_device.h) compiled for
// the host, so that a machine without a GPU can hold them against the oracle's (tests/cpp/prox_record_ref.cpp).
//
// Built at test time as a shared library, with the stand-in <hip/hip_runtime.h> of tests/cpp/hip_host first on the path:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I tests/cpp/hip_host -I include tests/cpp/prox_record_host.cpp
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

// the routine createProxFinderList gives the pair of kinds (0: no finder), and whether a is its shape1
int prh_pair_routine(int kind_a, int kind_b, int* a_is_shape1) {
  bool first = true;
  const int r = rkh::pair_routine(kind_a, kind_b, &first);
  *a_is_shape1 = first ? 1 : 0;
  return r;
}

// B pairs of world-anchored shapes in the finder's (shape1, shape2) order: [p1 (3), p2 (3), the record's distance,
// pair_distance's distance] each
void prh_pair_records(const rkh_shape* a, const rkh_shape* b, int routine, int B, double* out) {
  for (int i = 0; i < B; ++i) {
    const rkh::ShapeG s1 = posed(a[i]), s2 = posed(b[i]);
    const rkh::ProxRecordG r = rkh::pair_record(routine, s1, s2);
    double* o = out + 8 * i;
    o[0] = r.p1.x; o[1] = r.p1.y; o[2] = r.p1.z;
    o[3] = r.p2.x; o[4] = r.p2.y; o[5] = r.p2.z;
    o[6] = r.dist;
    o[7] = rkh::pair_distance<false>(routine, s1, s2);
  }
}

}  // extern "C"
