// proximity_record_device.h -- the closed-form pair routines of ReaK's geometry/proximity with their closest points:
// proximity_finder_3D::computeProximity filling a proximity_record_3D (mPoint1 on shape1, mPoint2 on shape2, both in the
// world frame, and mDistance; proximity_record_3D.hpp:47-56).
//
// proximity_device.h produces the distance alone, which is all a collision verdict needs; the record queries
// (rkh_min_distance_records, rkh_collision_records) find their pairs with those routines and then evaluate the forms
// below for the pairs they report.  Same branch structure and fp64 operation order as the reference routines
// (reference paths are relative to src/ReaK/geometry/proximity/):
//   prox_sphere_sphere.cpp:41-58, prox_sphere_ccylinder.cpp:43-80, prox_sphere_box.cpp:45-68,
//   prox_ccylinder_ccylinder.cpp:43-128, prox_ccylinder_box.cpp:45-70, prox_plane_plane.cpp:43-183,
//   prox_plane_sphere.cpp:106-122, prox_plane_ccylinder.cpp:43-74, prox_plane_cylinder.cpp:42-78,
//   prox_plane_box.cpp:43-71, prox_sphere_cylinder.cpp:43-92,
//   findProximityBoxToPoint / findProximityBoxToLine (prox_fundamentals_3D.cpp:35-115).
// Nothing here uses a device builtin: with a stand-in for <hip/hip_runtime.h> that defines __device__ and
// __forceinline__ a host compiler reads this header, proximity_device.h and device_math.h as they are
// (tests/cpp/prox_record_host.cpp).
#pragma once
#include "proximity_device.h"
#include "epa_device.h"

namespace rkh {

struct ProxRecordG {  // proximity_record_3D
  d3 p1, p2;
  double dist;
};

// findProximityBoxToPoint (prox_fundamentals_3D.cpp:35-82): p1 = the point of the box, p2 = the query point
RKH_DI ProxRecordG box_point_record(const ShapeG& bx, d3 pt) {
  const d3 p = pose_from_parent(bx.pos, bx.q, pt);
  const double hx = 0.5 * bx.d0, hy = 0.5 * bx.d1, hz = 0.5 * bx.d2;
  bool in_x = (p.x > -hx) && (p.x < hx);
  bool in_y = (p.y > -hy) && (p.y < hy);
  bool in_z = (p.z > -hz) && (p.z < hz);
  const bool inside = in_x && in_y && in_z;
  if (inside) {
    const double bx_ = hx - fabs(p.x), by_ = hy - fabs(p.y), bz_ = hz - fabs(p.z);
    if ((bx_ <= by_) && (bx_ <= bz_)) in_x = false;
    else if ((by_ <= bx_) && (by_ <= bz_)) in_y = false;
    else in_z = false;
  }
  d3 c = mk3(hx, hy, hz);
  if (in_x) c.x = p.x;
  else if (p.x < 0.0) c.x = -c.x;
  if (in_y) c.y = p.y;
  else if (p.y < 0.0) c.y = -c.y;
  if (in_z) c.z = p.z;
  else if (p.z < 0.0) c.z = -c.z;
  ProxRecordG r;
  r.p1 = pose_to_parent(bx.pos, bx.q, c);
  const double diff_d = norm_2(c - p);
  r.p2 = pt;
  r.dist = inside ? -diff_d : diff_d;
  return r;
}

// findProximityBoxToLine (prox_fundamentals_3D.cpp:108-115): the functor keeps the record of its last call, and the
// last call of golden_section_search_impl (line_search.hpp:74-95) is f((low + up) / 2).  The bracket moves on the
// distances alone, so the walk is box_line_distance's and only its last point is evaluated with its points.
RKH_DI ProxRecordG box_line_record(const ShapeG& bx, d3 center, d3 tangent, double half_len) {
  const double phi = 1.618033988;
  const double tol = 1e-3 * half_len;
  double low = -half_len, up = half_len;
  double mid = low + (up - low) / phi;
  double mid_cost = box_point_distance(bx, center + tangent * mid);
  for (int it = 0;; ++it) {
    if (fabs(low - up) < tol || it >= RKH_GOLDEN_MAX_ITER) return box_point_record(bx, center + tangent * ((low + up) * 0.5));
    const double test = mid + (up - mid) / phi;
    const double test_cost = box_point_distance(bx, center + tangent * test);
    if (test_cost < mid_cost) {
      low = mid;
      mid = test;
      mid_cost = test_cost;
    } else {
      up = low;
      low = test;
    }
  }
}

RKH_DI ProxRecordG rec_sphere_sphere(const ShapeG& s1, const ShapeG& s2) {  // prox_sphere_sphere.cpp:41-58
  ProxRecordG r;
  const d3 c1 = pose_to_parent(s1.pos, s1.q, mk3(0, 0, 0));
  const d3 c2 = pose_to_parent(s2.pos, s2.q, mk3(0, 0, 0));
  const d3 diff_cc = c2 - c1;
  const double dist_cc = norm_2(diff_cc);
  r.dist = dist_cc - s1.d0 - s2.d0;
  r.p1 = c1 + (s1.d0 / dist_cc) * diff_cc;
  r.p2 = c2 - (s2.d0 / dist_cc) * diff_cc;
  return r;
}

// prox_sphere_box.cpp:45-68 and prox_ccylinder_box.cpp:45-70 end alike: from the record of the box against the sphere's
// centre (the capped cylinder's axis point), step the radius towards the box, or away from it if the point is inside
RKH_DI ProxRecordG rec_round_box(const ProxRecordG& bxpt, double radius) {
  ProxRecordG r;
  const d3 diff_v = bxpt.p1 - bxpt.p2;
  const double diff_d = norm_2(diff_v);
  if (bxpt.dist < 0.0) r.p1 = bxpt.p2 - (radius / diff_d) * diff_v;
  else r.p1 = bxpt.p2 + (radius / diff_d) * diff_v;
  r.p2 = bxpt.p1;
  r.dist = bxpt.dist - radius;
  return r;
}

RKH_DI ProxRecordG rec_sphere_box(const ShapeG& sp, const ShapeG& bx) {
  const d3 sp_c = pose_to_parent(sp.pos, sp.q, mk3(0, 0, 0));
  return rec_round_box(box_point_record(bx, sp_c), sp.d0);
}

RKH_DI ProxRecordG rec_ccyl_box(const ShapeG& cc, const ShapeG& bx) {
  const d3 cy_c = pose_to_parent(cc.pos, cc.q, mk3(0, 0, 0));
  const d3 cy_t = qrot(cc.q, mk3(0.0, 0.0, 1.0));
  return rec_round_box(box_line_record(bx, cy_c, cy_t, 0.5 * cc.d0), cc.d1);
}

RKH_DI ProxRecordG rec_sphere_ccyl(const ShapeG& sp, const ShapeG& cc) {  // prox_sphere_ccylinder.cpp:43-80
  ProxRecordG r;
  const double len = cc.d0, rad = cc.d1, sr = sp.d0;
  const d3 sp_c = pose_to_parent(sp.pos, sp.q, mk3(0, 0, 0));
  const d3 rel = pose_from_parent(cc.pos, cc.q, sp_c);
  if (fabs(rel.z) <= 0.5 * len) {
    const d3 proj = mk3(rel.x, rel.y, 0.0);
    const double proj_d = norm_2(proj);
    r.p2 = pose_to_parent(cc.pos, cc.q, mk3(0.0, 0.0, rel.z) + proj * (rad / proj_d));
    r.p1 = pose_to_parent(cc.pos, cc.q, rel - proj * (sr / proj_d));
    r.dist = proj_d - sr - rad;
    return r;
  }
  double fact = 1.0;
  if (rel.z < 0.0) fact = -1.0;
  const d3 cy_c2 = pose_to_parent(cc.pos, cc.q, mk3(0.0, 0.0, fact * 0.5 * len));
  const d3 diff_cc = cy_c2 - sp_c;
  const double dist_cc = norm_2(diff_cc);
  r.dist = dist_cc - sr - rad;
  r.p1 = sp_c + (sr / dist_cc) * diff_cc;
  r.p2 = cy_c2 - (rad / dist_cc) * diff_cc;
  return r;
}

// prox_ccylinder_ccylinder.cpp:43-128 (the parallel branch's overlap test, :61-62, is a logical OR in the reference)
RKH_DI ProxRecordG rec_ccyl_ccyl(const ShapeG& c1, const ShapeG& c2) {
  ProxRecordG r;
  const double L1 = c1.d0, R1 = c1.d1, L2 = c2.d0, R2 = c2.d1;
  const d3 cy2_c = pose_to_parent(c2.pos, c2.q, mk3(0, 0, 0));
  const d3 cy2_t = qrot(c2.q, mk3(0.0, 0.0, 1.0));
  const d3 cr = pose_from_parent(c1.pos, c1.q, cy2_c);
  const d3 tr = qrot(qinv(c1.q), cy2_t);
  d3 p1, p2;  // the axis points, in capped cylinder 1's frame
  if (sqrt(tr.x * tr.x + tr.y * tr.y) < 1e-5) {
    if ((cr.z + 0.5 * L2 > -0.5 * L1) || (cr.z - 0.5 * L2 < 0.5 * L1)) {
      const double max_z = (cr.z + 0.5 * L2 < 0.5 * L1) ? (cr.z + 0.5 * L2) : (0.5 * L1);
      const double min_z = (cr.z - 0.5 * L2 > -0.5 * L1) ? (cr.z - 0.5 * L2) : (-0.5 * L1);
      const double avg_z = (max_z + min_z) * 0.5;
      const d3 rad_v = mk3(cr.x, cr.y, 0.0);
      const double rad_n = norm_2(rad_v);
      const d3 rr = mk3(rad_v.x / rad_n, rad_v.y / rad_n, rad_v.z / rad_n);  // unit(): vect_alg.hpp:2378-2382
      r.p1 = pose_to_parent(c1.pos, c1.q, mk3(R1 * rr.x, R1 * rr.y, avg_z));
      r.p2 = pose_to_parent(c1.pos, c1.q, mk3(cr.x - R2 * rr.x, cr.y - R2 * rr.y, avg_z));
      r.dist = sqrt(cr.x * cr.x + cr.y * cr.y) - R1 - R2;
      return r;
    }
    p1 = mk3(0.0, 0.0, 0.0);
    p2 = cr;
    if (cr.z < 0.0) {
      p1.z -= 0.5 * L1;
      p2.z += 0.5 * L2;
    } else {
      p1.z += 0.5 * L1;
      p2.z -= 0.5 * L2;
    }
  } else {
    const double d = dot(tr, cr);
    const double denom = 1.0 - tr.z * tr.z;
    double s_c = (tr.z * cr.z - d) / denom;
    double t_c = (cr.z - tr.z * d) / denom;
    if (s_c < -0.5 * L2) {
      s_c = -0.5 * L2;
      t_c = cr.z - 0.5 * L2 * tr.z;
    } else if (s_c > 0.5 * L2) {
      s_c = 0.5 * L2;
      t_c = cr.z + 0.5 * L2 * tr.z;
    }
    if (t_c < -0.5 * L1) {
      t_c = -0.5 * L1;
      s_c = -0.5 * L1 * tr.z - d;
    } else if (t_c > 0.5 * L1) {
      t_c = 0.5 * L1;
      s_c = 0.5 * L1 * tr.z - d;
    }
    if (s_c < -0.5 * L2) s_c = -0.5 * L2;
    else if (s_c > 0.5 * L2) s_c = 0.5 * L2;
    p1 = mk3(0.0, 0.0, t_c);
    p2 = cr + s_c * tr;
  }
  const d3 diff_v = p2 - p1;
  const double dist_v = norm_2(diff_v);
  r.p1 = pose_to_parent(c1.pos, c1.q, p1 + (R1 / dist_v) * diff_v);
  r.p2 = pose_to_parent(c1.pos, c1.q, p2 - (R2 / dist_v) * diff_v);
  r.dist = dist_v - R1 - R2;
  return r;
}

// ---- plane / cylinder finders: the plane is infinite (normal = local z) except in prox_plane_plane --------------------

// the foot on the plane of a point given in the plane's frame, and that point: the end of every prox_plane_* routine
RKH_DI ProxRecordG rec_plane_foot(const ShapeG& pl, d3 pt_rel) {
  ProxRecordG r;
  r.p1 = pose_to_parent(pl.pos, pl.q, mk3(pt_rel.x, pt_rel.y, 0.0));
  r.p2 = pose_to_parent(pl.pos, pl.q, pt_rel);
  r.dist = pt_rel.z;
  return r;
}

RKH_DI ProxRecordG rec_plane_sphere(const ShapeG& pl, const ShapeG& sp) {  // prox_plane_sphere.cpp:106-122
  const d3 sp_c = pose_to_parent(sp.pos, sp.q, mk3(0, 0, 0));
  const d3 rel = pose_from_parent(pl.pos, pl.q, sp_c);
  return rec_plane_foot(pl, mk3(rel.x, rel.y, rel.z - sp.d0));
}

// prox_plane_box.cpp:43-71: bx_x, bx_y and bx_z are ALL built from the box's local x axis in the reference (:53-55)
RKH_DI ProxRecordG rec_plane_box(const ShapeG& pl, const ShapeG& bx) {
  const d3 bx_c = pose_to_parent(bx.pos, bx.q, mk3(0, 0, 0));
  d3 bx_x = qrot(qinv(pl.q), qrot(bx.q, mk3(1.0, 0.0, 0.0)));
  if (bx_x.z > 0.0) bx_x = -bx_x;
  const d3 bx_y = bx_x, bx_z = bx_x;
  const d3 c_rel = pose_from_parent(pl.pos, pl.q, bx_c);
  return rec_plane_foot(pl, c_rel + 0.5 * (bx.d0 * bx_x + bx.d1 * bx_y + bx.d2 * bx_z));
}

RKH_DI ProxRecordG rec_plane_ccyl(const ShapeG& pl, const ShapeG& cc) {  // prox_plane_ccylinder.cpp:43-74
  const d3 cy_c = pose_to_parent(cc.pos, cc.q, mk3(0, 0, 0));
  const d3 cy_t = qrot(cc.q, mk3(0.0, 0.0, 1.0));
  const d3 c_rel = pose_from_parent(pl.pos, pl.q, cy_c);
  d3 t_rel = qrot(qinv(pl.q), cy_t);
  if (fabs(t_rel.z) < 1e-6) return rec_plane_foot(pl, mk3(c_rel.x, c_rel.y, c_rel.z - cc.d1));
  if (t_rel.z > 0.0) t_rel = -t_rel;
  return rec_plane_foot(pl, c_rel + (0.5 * cc.d0) * t_rel + mk3(0.0, 0.0, -cc.d1));
}

RKH_DI ProxRecordG rec_plane_cyl(const ShapeG& pl, const ShapeG& cy) {  // prox_plane_cylinder.cpp:42-78
  const d3 cy_c = pose_to_parent(cy.pos, cy.q, mk3(0, 0, 0));
  const d3 cy_t = qrot(cy.q, mk3(0.0, 0.0, 1.0));
  const d3 c_rel = pose_from_parent(pl.pos, pl.q, cy_c);
  d3 t_rel = qrot(qinv(pl.q), cy_t);
  if (fabs(t_rel.z) < 1e-6) return rec_plane_foot(pl, mk3(c_rel.x, c_rel.y, c_rel.z - cy.d1));
  if (sqrt(t_rel.x * t_rel.x + t_rel.y * t_rel.y) < 1e-6) return rec_plane_foot(pl, mk3(c_rel.x, c_rel.y, c_rel.z - 0.5 * cy.d0));
  if (t_rel.z > 0.0) t_rel = -t_rel;
  const d3 v = mk3(0.0, 0.0, -1.0) + t_rel.z * t_rel;
  const double n = norm_2(v);
  const d3 r_rel = mk3(v.x / n, v.y / n, v.z / n);  // unit(): vect_alg.hpp:2378-2382
  return rec_plane_foot(pl, c_rel + (0.5 * cy.d0) * t_rel + cy.d1 * r_rel);
}

// prox_plane_plane::computeProximityOfPoint (prox_plane_plane.cpp:43-95): here the plane is finite.  p1 = the point of
// the plane, p2 = the query point.
RKH_DI ProxRecordG plane_point_record(const ShapeG& pl, d3 pt) {
  ProxRecordG r;
  r.p2 = pt;
  const d3 p = pose_from_parent(pl.pos, pl.q, pt);
  const double hx = 0.5 * pl.d0, hy = 0.5 * pl.d1;
  const bool in_x = (p.x > -hx) && (p.x < hx), in_y = (p.y > -hy) && (p.y < hy);
  if (in_x && in_y) {
    double fact = 1.0;
    if (p.z < 0.0) fact = -1.0;
    r.p1 = pose_to_parent(pl.pos, pl.q, mk3(p.x, p.y, 0.0));
    r.dist = fact * p.z;
    return r;
  }
  d3 rim;
  if (in_x) {
    double fact = 1.0;
    if (p.y < 0.0) fact = -1.0;
    rim = mk3(p.x, fact * 0.5 * pl.d1, 0.0);
  } else if (in_y) {
    double fact = 1.0;
    if (p.x < 0.0) fact = -1.0;
    rim = mk3(fact * 0.5 * pl.d0, p.y, 0.0);
  } else {
    rim = mk3(0.5 * pl.d0, 0.5 * pl.d1, 0.0);
    if (p.x < 0.0) rim.x = -rim.x;
    if (p.y < 0.0) rim.y = -rim.y;
  }
  r.p1 = pose_to_parent(pl.pos, pl.q, rim);
  r.dist = norm_2(r.p1 - pt);
  return r;
}

// prox_plane_plane.cpp:98-183: the corners of plane 2 against plane 1, then those of plane 1 against plane 2; a later
// corner replaces the record only if it is strictly closer
RKH_DI ProxRecordG rec_plane_plane(const ShapeG& p1, const ShapeG& p2) {
  ProxRecordG best;
  best.p1 = best.p2 = mk3(0.0, 0.0, 0.0);
  best.dist = INFINITY;
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    const ShapeG& of = side == 0 ? p2 : p1;
    const ShapeG& against = side == 0 ? p1 : p2;
    d3 corner = mk3(0.5 * of.d0, 0.5 * of.d1, 0.0);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      if (k == 1 || k == 3) corner.y = -corner.y;
      if (k == 2) corner.x = -corner.x;
      const ProxRecordG c = plane_point_record(against, pose_to_parent(of.pos, of.q, corner));
      if (c.dist < best.dist) {
        best.dist = c.dist;
        best.p1 = side == 0 ? c.p1 : c.p2;
        best.p2 = side == 0 ? c.p2 : c.p1;
      }
    }
  }
  return best;
}

RKH_DI ProxRecordG rec_sphere_cyl(const ShapeG& sp, const ShapeG& cy) {  // prox_sphere_cylinder.cpp:43-92
  ProxRecordG r;
  const double L = cy.d0, R = cy.d1, sr = sp.d0;
  const d3 sp_c = pose_to_parent(sp.pos, sp.q, mk3(0, 0, 0));
  const d3 rel = pose_from_parent(cy.pos, cy.q, sp_c);
  const double rel_rad = sqrt(rel.x * rel.x + rel.y * rel.y);
  if (fabs(rel.z) <= 0.5 * L) {
    const d3 proj = mk3(rel.x, rel.y, 0.0);
    const double proj_d = norm_2(proj);
    r.p2 = pose_to_parent(cy.pos, cy.q, mk3(0.0, 0.0, rel.z) + proj * (R / proj_d));
    r.p1 = pose_to_parent(cy.pos, cy.q, rel - proj * (sr / proj_d));
    r.dist = proj_d - sr - R;
    return r;
  }
  double fact = 1.0;
  if (rel.z < 0.0) fact = -1.0;
  if (rel_rad < R) {
    r.p2 = pose_to_parent(cy.pos, cy.q, mk3(rel.x, rel.y, fact * 0.5 * L));
    r.p1 = pose_to_parent(cy.pos, cy.q, mk3(rel.x, rel.y, rel.z - fact * sr));
    r.dist = fact * rel.z - 0.5 * L - sr;
    return r;
  }
  const d3 proj = mk3(rel.x, rel.y, 0.0);
  const double proj_d = norm_2(proj);
  const d3 rim = (R / proj_d) * proj + mk3(0.0, 0.0, fact * 0.5 * L);
  r.p2 = pose_to_parent(cy.pos, cy.q, rim);
  const d3 to_rim = r.p2 - sp_c;
  const double to_rim_d = norm_2(to_rim);
  r.p1 = sp_c + (sr / to_rim_d) * to_rim;
  r.dist = to_rim_d - sr;
  return r;
}

// (shape1, shape2) in the routine's own argument order, as for pair_distance.  This form knows the closed forms only:
// vertex-set pairs (PR_GJK) get no record from it, and the plain record queries refuse scenes that hold such shapes.
RKH_DI ProxRecordG pair_record(int routine, const ShapeG& s1, const ShapeG& s2) {
  switch (routine) {
    case PR_SPHERE_SPHERE: return rec_sphere_sphere(s1, s2);
    case PR_SPHERE_CCYL: return rec_sphere_ccyl(s1, s2);
    case PR_SPHERE_BOX: return rec_sphere_box(s1, s2);
    case PR_CCYL_CCYL: return rec_ccyl_ccyl(s1, s2);
    case PR_CCYL_BOX: return rec_ccyl_box(s1, s2);
    case PR_PLANE_PLANE: return rec_plane_plane(s1, s2);
    case PR_PLANE_SPHERE: return rec_plane_sphere(s1, s2);
    case PR_PLANE_CCYL: return rec_plane_ccyl(s1, s2);
    case PR_PLANE_CYL: return rec_plane_cyl(s1, s2);
    case PR_PLANE_BOX: return rec_plane_box(s1, s2);
    case PR_SPHERE_CYL: return rec_sphere_cyl(s1, s2);
  }
  ProxRecordG none;
  none.p1 = none.p2 = mk3(0.0, 0.0, 0.0);
  none.dist = INFINITY;
  return none;
}

// The same with the scene's vertex pool.  GJK = true answers vertex-set pairs too, with the witnesses of the support-map
// search (gjk_record: shape1 = model 1's shape, as pair_routine orders a PR_GJK pair); GJK = false is the form above.
template <bool GJK = false>
RKH_DI ProxRecordG pair_record(int routine, const ShapeG& s1, const ShapeG& s2, const double* mesh_pool) {
  if (GJK) {
    if (routine == PR_GJK) {
      const GjkRecord g = gjk_record(to_gjk(s1, mesh_pool), to_gjk(s2, mesh_pool));
      ProxRecordG r;
      r.p1 = g.p1;
      r.p2 = g.p2;
      r.dist = g.dist;
      return r;
    }
  }
  return pair_record(routine, s1, s2);
}

// ---- the third mode: records with a penetration depth and a normal (the *_depth entries) -------------------------------
// Vertex-set pairs (PR_GJK) go through gjk_depth_distance / gjk_depth_record of epa_device.h: where the cores cross, dist
// is -(r1 + r2 + depth) - kGjkOverlap and nrm the contact normal; where they are apart, gjk_distance's / gjk_record's
// values.  Every other pair is the closed form above, unchanged, with nrm = (point2 - point1) / dist componentwise
// (zeros where dist is 0 or not finite); no more is claimed for those.
struct ProxRecordN {
  d3 p1, p2, nrm;
  double dist;
};

RKH_DI double pair_distance_depth(int routine, const ShapeG& s1, const ShapeG& s2, const double* mesh_pool) {
  if (routine == PR_GJK) return gjk_depth_distance(to_gjk(s1, mesh_pool), to_gjk(s2, mesh_pool));
  return pair_distance<false>(routine, s1, s2);
}

RKH_DI ProxRecordN pair_record_depth(int routine, const ShapeG& s1, const ShapeG& s2, const double* mesh_pool) {
  ProxRecordN r;
  if (routine == PR_GJK) {
    const GjkDepthRecord g = gjk_depth_record(to_gjk(s1, mesh_pool), to_gjk(s2, mesh_pool));
    r.p1 = g.p1;
    r.p2 = g.p2;
    r.nrm = g.nrm;
    r.dist = g.dist;
    return r;
  }
  const ProxRecordG c = pair_record(routine, s1, s2);
  r.p1 = c.p1;
  r.p2 = c.p2;
  r.dist = c.dist;
  const bool usable = c.dist != 0.0 && fabs(c.dist) < INFINITY;  // (a NaN fails both)
  const d3 diff = c.p2 - c.p1;
  r.nrm = usable ? mk3(diff.x / c.dist, diff.y / c.dist, diff.z / c.dist) : mk3(0.0, 0.0, 0.0);
  return r;
}

}  // namespace rkh
