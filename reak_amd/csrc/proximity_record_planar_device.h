// proximity_record_planar_device.h -- the closed-form planar (2D) pair routines of ReaK's geometry/proximity with their
// closest points: proximity_finder_2D::computeProximity filling a proximity_record_2D (mPoint1 on shape1, mPoint2 on
// shape2, both in the world frame, and mDistance; proximity_record_2D.hpp:47-58).
//
// proximity_planar_device.h produces the distance alone, which is all a verdict needs; the planar record queries
// (rkh_min_distance_records_2d, rkh_collision_records_2d) find their pairs with those routines and then evaluate the
// forms below for the pairs they report.  Same branch structure and fp64 operation order as the distance-only forms and
// as the reference routines (relative to src/ReaK/geometry/proximity/):
//   prox_circle_circle.cpp:40-57, prox_circle_crect.cpp:40-84, prox_circle_rectangle.cpp:40-86,
//   prox_crect_crect.cpp:40-131, prox_crect_rectangle.cpp:40-205, prox_rectangle_rectangle.cpp:40-168.
// The quirks of the reference stay: the overlap tests of the parallel branches are '||' and always true, and
// circle / rectangle measures from the centre to the rectangle's boundary whichever side of it the centre is on (never
// below -radius).  Every form's distance is pair_distance_planar's bit for bit.
// Nothing here uses a device builtin: with a stand-in for <hip/hip_runtime.h> that defines __device__ and
// __forceinline__ a host compiler reads this header, proximity_planar_device.h and device_math.h as they are
// (tests/cpp/prox_record_host_2d.cpp).
#pragma once
#include "proximity_planar_device.h"

namespace rkh {

struct ProxRecordP {  // proximity_record_2D
  d2 p1, p2;
  double dist;
};

RKH_DI ProxRecordP rec_circle_circle(const ShapeP& s1, const ShapeP& s2) {
  const d2 c1 = to_parent(s1, mk2(0.0, 0.0)), c2 = to_parent(s2, mk2(0.0, 0.0));
  const d2 diff_cc = c2 - c1;
  const double dist_cc = norm_2(diff_cc);
  ProxRecordP r;
  r.dist = dist_cc - s1.d0 - s2.d0;
  r.p1 = c1 + (s1.d0 / dist_cc) * diff_cc;
  r.p2 = c2 - (s2.d0 / dist_cc) * diff_cc;
  return r;
}

RKH_DI ProxRecordP rec_circle_crect(const ShapeP& ci, const ShapeP& cr) {
  const d2 rel = from_parent(cr, to_parent(ci, mk2(0.0, 0.0)));
  const double R = ci.d0;
  ProxRecordP r;
  if ((rel.x > -0.5 * cr.d0) && (rel.x < 0.5 * cr.d0)) {  // beside the straight sides
    if (rel.y > 0.0) {
      r.p1 = to_parent(cr, mk2(rel.x, rel.y - R));
      r.p2 = to_parent(cr, mk2(rel.x, 0.5 * cr.d1));
      r.dist = rel.y - R - 0.5 * cr.d1;
    } else {
      r.p1 = to_parent(cr, mk2(rel.x, rel.y + R));
      r.p2 = to_parent(cr, mk2(rel.x, -0.5 * cr.d1));
      r.dist = -0.5 * cr.d1 - rel.y - R;
    }
    return r;
  }
  d2 endc = mk2(0.0, 0.0);
  if (rel.x > 0.0) endc.x += 0.5 * cr.d0;
  else endc.x -= 0.5 * cr.d0;
  const d2 diff = rel - endc;
  const double dd = norm_2(diff);
  r.p1 = to_parent(cr, rel - (R / dd) * diff);
  r.p2 = to_parent(cr, endc + (0.5 * cr.d1 / dd) * diff);
  r.dist = dd - 0.5 * cr.d1 - R;
  return r;
}

RKH_DI ProxRecordP rec_circle_rect(const ShapeP& ci, const ShapeP& re) {
  const d2 ci_c = to_parent(ci, mk2(0.0, 0.0));
  ProxRecordP r;
  r.p2 = to_parent(re, rect_corner_point(re, from_parent(re, ci_c)));
  const d2 diff = r.p2 - ci_c;
  const double dd = norm_2(diff);
  r.p1 = ci_c + (ci.d0 / dd) * diff;
  r.dist = dd - ci.d0;  // |centre - boundary point| - radius, also for a centre inside the rectangle
  return r;
}

RKH_DI ProxRecordP rec_crect_crect(const ShapeP& c1, const ShapeP& c2) {
  const d2 c2c = to_parent(c2, mk2(0.0, 0.0));
  const d2 c2t = rrot(c2.rot, mk2(1.0, 0.0));
  const d2 cr = from_parent(c1, c2c);
  const d2 tr = rrotT(c2t, c1.rot);
  const double L1 = c1.d0, W1 = c1.d1, L2 = c2.d0, W2 = c2.d1;
  ProxRecordP r;
  d2 a, b;  // the two centre-line points, in c1's frame
  if (fabs(tr.y) < 1e-5) {  // parallel centre lines
    if ((cr.x + 0.5 * L2 > -0.5 * L1) || (cr.x - 0.5 * L2 < 0.5 * L1)) {  // always true (:58-59)
      const double max_x = (cr.x + 0.5 * L2 < 0.5 * L1) ? (cr.x + 0.5 * L2) : (0.5 * L1);
      const double min_x = (cr.x - 0.5 * L2 > -0.5 * L1) ? (cr.x - 0.5 * L2) : (-0.5 * L1);
      const double avg_x = (max_x + min_x) * 0.5;
      const double side = (cr.y < 0.0) ? -1.0 : 1.0;
      r.p1 = to_parent(c1, mk2(avg_x, 0.5 * W1 * side));
      r.p2 = to_parent(c1, mk2(avg_x, cr.y - 0.5 * W2 * side));
      r.dist = fabs(cr.y) - 0.5 * W1 - 0.5 * W2;
      return r;
    }
    a = mk2(0.0, 0.0);
    b = cr;
    if (cr.x < 0.0) {
      a.x -= 0.5 * L1;
      b.x += 0.5 * L2;
    } else {
      a.x += 0.5 * L1;
      b.x -= 0.5 * L2;
    }
  } else {
    const double d = dot(tr, cr);
    const double denom = 1.0 - tr.x * tr.x;
    double s_c = (tr.x * cr.x - d) / denom;
    double t_c = (cr.x - tr.x * d) / denom;
    if (s_c < -0.5 * L2) {
      s_c = -0.5 * L2;
      t_c = cr.x - 0.5 * L2 * tr.x;
    } else if (s_c > 0.5 * L2) {
      s_c = 0.5 * L2;
      t_c = cr.x + 0.5 * L2 * tr.x;
    }
    if (t_c < -0.5 * L1) {
      t_c = -0.5 * L1;
      s_c = -0.5 * L1 * tr.x - d;
    } else if (t_c > 0.5 * L1) {
      t_c = 0.5 * L1;
      s_c = 0.5 * L1 * tr.x - d;
    }
    if (s_c < -0.5 * L2) s_c = -0.5 * L2;
    else if (s_c > 0.5 * L2) s_c = 0.5 * L2;
    a = mk2(t_c, 0.0);
    b = cr + s_c * tr;
  }
  const d2 diff = b - a;
  const double dd = norm_2(diff);
  r.p1 = to_parent(c1, a + (0.5 * W1 / dd) * diff);
  r.p2 = to_parent(c1, b - (0.5 * W2 / dd) * diff);
  r.dist = dd - 0.5 * W1 - 0.5 * W2;
  return r;
}

// prox_crect_rectangle: the centre line against the rectangle (computeProximityOfLine, :40-181), then the circle sweep
// (:184-205), which moves mPoint1 along the line between the two points by half the width
RKH_DI ProxRecordP rec_crect_rect(const ShapeP& cr, const ShapeP& re) {
  const d2 ln_c = to_parent(cr, mk2(0.0, 0.0));
  const d2 ln_t = rrot(cr.rot, mk2(1.0, 0.0));
  const double half_length = 0.5 * cr.d0;
  const d2 c = from_parent(re, ln_c);
  const d2 t = rrotT(ln_t, re.rot);
  const double DX = re.d0, DY = re.d1;
  double dist;
  d2 ln_pt, re_pt;  // in the rectangle's frame
  if (fabs(t.x) < 1e-5) {  // vertical line
    if ((c.y + half_length > -0.5 * DY) || (c.y - half_length < 0.5 * DY)) {  // always true (:51-52)
      const double max_y = (c.y + half_length < 0.5 * DY) ? (c.y + half_length) : (0.5 * DY);
      const double min_y = (c.y - half_length > -0.5 * DY) ? (c.y - half_length) : (-0.5 * DY);
      const double avg_y = (max_y + min_y) * 0.5;
      const double side = (c.x < 0.0) ? -1.0 : 1.0;
      ln_pt = mk2(c.x, avg_y);
      re_pt = mk2(0.5 * DX * side, avg_y);
      dist = fabs(c.x) - 0.5 * DX;
    } else {
      re_pt = mk2(0.0, 0.0);
      ln_pt = c;
      if (c.x < 0.0) re_pt.x -= 0.5 * DX;
      else re_pt.x += 0.5 * DX;
      if (c.y < 0.0) {
        re_pt.y -= 0.5 * DY;
        ln_pt.y += half_length;
      } else {
        re_pt.y += 0.5 * DY;
        ln_pt.y -= half_length;
      }
      dist = norm_2(ln_pt - re_pt);
    }
  } else if (fabs(t.y) < 1e-5) {  // horizontal line
    if ((c.x + half_length > -0.5 * DX) || (c.x - half_length < 0.5 * DX)) {  // always true (:90-91)
      const double max_x = (c.x + half_length < 0.5 * DX) ? (c.x + half_length) : (0.5 * DX);
      const double min_x = (c.x - half_length > -0.5 * DX) ? (c.x - half_length) : (-0.5 * DX);
      const double avg_x = (max_x + min_x) * 0.5;
      const double side = (c.y < 0.0) ? -1.0 : 1.0;
      ln_pt = mk2(avg_x, c.y);
      re_pt = mk2(avg_x, 0.5 * DY * side);
      dist = fabs(c.y) - 0.5 * DY;
    } else {
      re_pt = mk2(0.0, 0.0);
      ln_pt = c;
      if (c.y < 0.0) re_pt.y -= 0.5 * DY;
      else re_pt.y += 0.5 * DY;
      if (c.x < 0.0) {
        re_pt.x -= 0.5 * DX;
        ln_pt.x += half_length;
      } else {
        re_pt.x += 0.5 * DX;
        ln_pt.x -= half_length;
      }
      dist = norm_2(ln_pt - re_pt);
    }
  } else {  // segment-point test (:126-180)
    d2 n = mk2(-t.y * 1.0, t.x * 1.0);  // 1.0 % ln_t_rel
    if (dot(n, c) < 0.0) n = -n;
    d2 corner = mk2(-0.5 * DX, -0.5 * DY);
    if (n.x > 0.0) corner.x = 0.5 * DX;
    if (n.y > 0.0) corner.y = 0.5 * DY;
    const d2 diff = c - corner;
    dist = dot(diff, n);
    double t_tmp = -dot(diff, t);
    if (fabs(t_tmp) > half_length) {
      if (t_tmp < 0.0) t_tmp = -half_length;
      else t_tmp = half_length;
      ln_pt = c + t_tmp * t;
      const double in_x = fabs(ln_pt.x) - 0.5 * DX;
      const double in_y = fabs(ln_pt.y) - 0.5 * DY;
      if ((in_x < 0.0) && (in_y > in_x)) {
        corner.x = ln_pt.x;
        dist = fabs(ln_pt.y) - 0.5 * DY;
      } else if ((in_y < 0.0) && (in_x > in_y)) {
        corner.y = ln_pt.y;
        dist = fabs(ln_pt.x) - 0.5 * DX;
      } else {
        if (ln_pt.x < 0.0) corner.x = -0.5 * DX;
        else corner.x = 0.5 * DX;
        if (ln_pt.y < 0.0) corner.y = -0.5 * DY;
        else corner.y = 0.5 * DY;
        dist = norm_2(ln_pt - corner);
      }
    } else {
      ln_pt = corner + dist * n;
    }
    re_pt = corner;
  }
  ProxRecordP r;
  r.p1 = to_parent(re, ln_pt);
  r.p2 = to_parent(re, re_pt);
  const d2 diff_v = r.p2 - r.p1;
  const double diff_d = norm_2(diff_v);
  if (dist < 0.0) r.p1 = r.p1 - (0.5 * cr.d1 / diff_d) * diff_v;
  else r.p1 = r.p1 + (0.5 * cr.d1 / diff_d) * diff_v;
  r.dist = dist - 0.5 * cr.d1;
  return r;
}

// prox_rectangle_rectangle (:79-168): the four corners of each rectangle against the other, first strict minimum wins
RKH_DI ProxRecordP rec_rect_rect(const ShapeP& r1, const ShapeP& r2) {
  ProxRecordP r;
  r.p1 = r.p2 = mk2(0.0, 0.0);
  r.dist = INFINITY;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const ShapeP& own = pass == 0 ? r2 : r1;
    const ShapeP& other = pass == 0 ? r1 : r2;
    d2 corner = mk2(own.d0 * 0.5, own.d1 * 0.5);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c == 1 || c == 3) corner.y = -corner.y;
      if (c == 2) corner.x = -corner.x;
      const d2 g = to_parent(own, corner);
      const d2 rec = to_parent(other, rect_corner_point(other, from_parent(other, g)));
      const double dd = norm_2(rec - g);
      if (dd < r.dist) {
        r.dist = dd;
        r.p1 = pass == 0 ? rec : g;
        r.p2 = pass == 0 ? g : rec;
      }
    }
  }
  return r;
}

RKH_DI ProxRecordP pair_record_planar(int routine, const ShapeP& s1, const ShapeP& s2) {
  switch (routine) {
    case PR_CIRCLE_CIRCLE: return rec_circle_circle(s1, s2);
    case PR_CIRCLE_CRECT: return rec_circle_crect(s1, s2);
    case PR_CIRCLE_RECT: return rec_circle_rect(s1, s2);
    case PR_CRECT_CRECT: return rec_crect_crect(s1, s2);
    case PR_CRECT_RECT: return rec_crect_rect(s1, s2);
    case PR_RECT_RECT: return rec_rect_rect(s1, s2);
  }
  ProxRecordP r;
  r.p1 = r.p2 = mk2(0.0, 0.0);
  r.dist = INFINITY;
  return r;
}

}  // namespace rkh
