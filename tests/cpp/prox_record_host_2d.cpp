// prox_record_host_2d.cpp -- the device's planar closed forms with points
// (reak_amd/csrc/proximity_record_planar_device.h) compiled for the host, so that a machine without a GPU can hold them
// against the oracle's (tests/cpp/prox_record_ref_2d.cpp).
//
// Built at test time as a shared library, with the stand-in <hip/hip_runtime.h> of tests/cpp/hip_host first on the path:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I tests/cpp/hip_host -I include tests/cpp/prox_record_host_2d.cpp
#include "../../reak_amd/csrc/proximity_record_planar_device.h"

#include "../../include/rkh_types.h"

namespace {
rkh::ShapeP posed(const rkh_shape& s) {
  rkh::ShapeP g;
  g.kind = s.kind;
  g.pos = rkh::mk2(s.pose.pos[0], s.pose.pos[1]);
  g.rot = rkh::mk2(s.pose.quat[0], s.pose.quat[1]);
  g.d0 = s.dims[0];
  g.d1 = s.dims[1];
  return g;
}
}  // namespace

extern "C" {

// B pairs of world-anchored shapes in the finder's (shape1, shape2) order: [p1 (2), p2 (2), the record's distance,
// pair_distance_planar's distance] each
void prh2_pair_records(const rkh_shape* a, const rkh_shape* b, int routine, int B, double* out) {
  for (int i = 0; i < B; ++i) {
    const rkh::ShapeP s1 = posed(a[i]), s2 = posed(b[i]);
    const rkh::ProxRecordP r = rkh::pair_record_planar(routine, s1, s2);
    double* o = out + 6 * i;
    o[0] = r.p1.x; o[1] = r.p1.y;
    o[2] = r.p2.x; o[3] = r.p2.y;
    o[4] = r.dist;
    o[5] = rkh::pair_distance_planar(routine, s1, s2);
  }
}

}  // extern "C"
