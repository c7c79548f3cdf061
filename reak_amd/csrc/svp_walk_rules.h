// svp_walk_rules.h -- the per-row scalar rules of the directed walk over the SVP space (svp_walk_dir.hip), as functions a
// host compiler reads too (tests/cpp/svp_walk_dir_host.cpp) and the Python twins restate (tests/svp_ref.py::edge_walk for a
// forward row, tests/svp_back_ref.py::edge_walk_back for a backward one).
//
// A row is the profile a -> b of reach time T, walked in one of two directions:
//   forward   move_pt_toward: the times min_interval, + min_interval, ... below dt = T fraction, from a; the last free point
//   backward  move_pt_back_to (svp_Ndof_reach_topologies.hpp:147-176): the times T - min_interval, - min_interval, ...
//             above dt = T (1 - fraction), from b; the last free point
// The rules: the count of points, the first time and the time j points later, the point a walk starts from, and what the
// row returns when no point fails.  Every time is made by adding or subtracting min_interval one at a time, so that its bits
// are the sequential loop's.  Only +, -, * and comparisons in fp64; nothing here uses a device builtin.
#pragma once
#include "svp_device.h"

namespace rkh {

constexpr uint32_t kSvpWalkPass = 32;             // points per live row and pass: the workspace of svp_walk_layout holds that many
constexpr uint32_t kSvpWalkMaxPoints = 1u << 20;  // tested points of one row (a walk that would test more is refused)

enum SvpWalkEnd : int { kSvpWalkEndA = 0, kSvpWalkEndB = 1, kSvpWalkEndPoint = 2 };

// the time the loop stops at: points are tested strictly before it (forward) or strictly after it (backward)
RKH_HD double svp_walk_dt(bool back, double T, double fraction) { return back ? T * (1.0 - fraction) : T * fraction; }

// the time of the first point
RKH_HD double svp_walk_first(bool back, double min_interval, double T) { return back ? T - min_interval : min_interval; }

// the time j points after d, one step at a time
RKH_HD double svp_walk_advance(bool back, double d, double min_interval, uint32_t j) {
  if (back)
    for (uint32_t c = 0; c < j; ++c) d -= min_interval;
  else
    for (uint32_t c = 0; c < j; ++c) d += min_interval;
  return d;
}

// is a point at time d still one of the loop's
RKH_HD bool svp_walk_open(bool back, double d, double dt) { return back ? (d > dt) : (d < dt); }

// Tested points of a row, counted by the same repeated addition or subtraction as the walk makes; at most cap (then *over
// is set: the caller refuses the row instead of looping for ever).
RKH_HD uint32_t svp_walk_count(bool back, double min_interval, double T, double dt, uint32_t cap, bool* over) {
  uint32_t k = 0;
  double d = svp_walk_first(back, min_interval, T);
  *over = false;
  while (svp_walk_open(back, d, dt)) {
    if (k == cap) {
      *over = true;
      break;
    }
    ++k;
    d = back ? d - min_interval : d + min_interval;
  }
  return k;
}

// the end of the profile a walk starts from (the "last free point" before any point is tested), and the one an infeasible
// pair returns: a forward, b backward
RKH_HD SvpWalkEnd svp_walk_origin(bool back) { return back ? kSvpWalkEndB : kSvpWalkEndA; }

// what a row returns when every tested point is free: the far end for fraction 1, the origin for 0, else the (untested)
// point of the profile at dt
RKH_HD SvpWalkEnd svp_walk_result(bool back, double fraction) {
  if (fraction == 1.0) return back ? kSvpWalkEndA : kSvpWalkEndB;
  if (fraction == 0.0) return back ? kSvpWalkEndB : kSvpWalkEndA;
  return kSvpWalkEndPoint;
}

}  // namespace rkh
