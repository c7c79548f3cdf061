// gjk_device.h -- GJK distance between convex shapes given by support maps (fp64), for the pairs the reference has no
// closed form for: everything that involves a CONVEX VERTEX SET ("mesh", RKH_SHAPE_MESH).
//
// The reference's proximity module has closed-form pairs only (no mesh shape, no GJK: TODO_list.txt:230); BASELINE
// config C4 asks for convex-mesh obstacles through "batched GJK / support-mapping distance queries".  This is the
// build's definition of that query, the same in the oracle (oracle/reak_gjk.hpp) and on the device:
//   * a shape = a convex CORE swept by a radius: sphere = point + r, capped cylinder = axis segment + r, box, mesh and
//     the flat-ended cylinder = themselves (r = 0; the cylinder's support map is curved, so its pairs end on the
//     relative tolerance or the iteration cap instead of a repeated vertex).  The radii are handled analytically (distance = core distance - rA - rB), so pairs of
//     spheres / capped cylinders / boxes reproduce the reference's closed forms to rounding while the cores are apart;
//   * core distance = Gilbert-Johnson-Keerthi on the Minkowski difference with polytope supports (finite termination),
//     closest point of the simplex by Voronoi-region tests (Ericson, Real-Time Collision Detection 5.1);
//   * termination: with v the closest point of the simplex and w the support point of A - B towards the origin,
//     v.w / |v| <= distance <= |v|.  |v| is returned only when CERTIFIED by that bound:
//         |v| - v.w / |v|  <=  kGjkRelTol |v| + kGjkAbsTol |w|
//     (the second term is the rounding of v.(v - w) itself, a few ulps of |v| |w|; it needs a v perpendicular to its
//     simplex to its OWN rounding, not to that of the far larger simplex points, hence gjk_foot and the normal form
//     in gjk_closest3).  An uncertified v gains the support point and the loop goes on; a tetrahedron too flat for
//     its side tests (kGjkFlat) takes the best of all four faces, so |v| never grows.  Where the loop cannot go on
//     -- the support point is in the simplex already, or kGjkMaxIter (reached by curved cores only) -- the result is
//     the lower bound max(v.w / |v|, 0) itself: below the distance by as much as the certificate missed, never above;
//   * intersecting cores: the penetration depth is not computed; the result is -(rA + rB) - kGjkOverlap (negative =
//     collision, which is all manip_dk_proxy_env_impl::is_free looks at, manip_free_workspace.hpp:85-95).
// Closed forms stay the default for primitive pairs (they ARE the reference); GJK runs for mesh pairs, and for any
// pair through the diagnostic entry point that checks it against the closed forms.
#pragma once
#include "../../include/rkh_types.h"
#include "device_math.h"

namespace rkh {

constexpr double kGjkOverlap = 1e-9;
constexpr int kGjkMaxIter = 64;
constexpr double kGjkRelTol = 1e-14;  // certified exit: relative part
constexpr double kGjkAbsTol = 1e-14;  // certified exit: rounding of v.(v - w), in units of |v| |w| (45 ulps)
constexpr double kGjkFlat = 1e-12;    // height / edge below which a tetrahedron's (a triangle's) orientation is rounding noise

struct GjkShape {
  int kind;
  d3 pos;
  m33 R;  // rotmat(q): local -> world
  double d0, d1, d2;
  const double* verts;  // mesh: nv local vertices (x, y, z), else unused
  int nv;
};

RKH_DI double gjk_radius(const GjkShape& s) {
  return s.kind == RKH_SHAPE_SPHERE ? s.d0 : (s.kind == RKH_SHAPE_CCYLINDER ? s.d1 : 0.0);
}

// support point of the shape's CORE in world direction dir
RKH_DI d3 gjk_support(const GjkShape& s, d3 dir) {
  const d3 dl = mulT(dir, s.R);  // R^T dir
  d3 p;
  if (s.kind == RKH_SHAPE_SPHERE) {
    p = mk3(0.0, 0.0, 0.0);
  } else if (s.kind == RKH_SHAPE_CCYLINDER) {
    p = mk3(0.0, 0.0, dl.z >= 0.0 ? 0.5 * s.d0 : -0.5 * s.d0);
  } else if (s.kind == RKH_SHAPE_BOX) {
    p = mk3(dl.x >= 0.0 ? 0.5 * s.d0 : -0.5 * s.d0, dl.y >= 0.0 ? 0.5 * s.d1 : -0.5 * s.d1,
            dl.z >= 0.0 ? 0.5 * s.d2 : -0.5 * s.d2);
  } else if (s.kind == RKH_SHAPE_CYLINDER) {  // flat-ended cylinder (d0 = length, d1 = radius; axis = local z): rim point
    const double rho = sqrt(dl.x * dl.x + dl.y * dl.y);
    p = mk3(rho > 0.0 ? (s.d1 * dl.x) / rho : 0.0, rho > 0.0 ? (s.d1 * dl.y) / rho : 0.0,
            dl.z >= 0.0 ? 0.5 * s.d0 : -0.5 * s.d0);
  } else {  // mesh: first maximum wins
    double best = -INFINITY;
    p = mk3(0.0, 0.0, 0.0);
#pragma unroll 1
    for (int i = 0; i < s.nv; ++i) {
      const d3 v = mk3(s.verts[3 * i], s.verts[3 * i + 1], s.verts[3 * i + 2]);
      const double t = dot(dl, v);
      if (t > best) {
        best = t;
        p = v;
      }
    }
  }
  return s.pos + mul(s.R, p);
}

// Foot of the origin on the line a + t ab, near the parameter t.  a + t ab alone carries the rounding of |a| along ab,
// which tilts a short v by |a| / |v| ulps; taking the component along ab out again leaves v perpendicular to the edge
// to its own rounding, which is what the certified exit of gjk_distance relies on.
RKH_DI d3 gjk_foot(d3 a, d3 ab, double t) {
  const d3 p = a + t * ab;
  return p - (dot(p, ab) / dot(ab, ab)) * ab;
}

// Closest point to the origin on the segment a, b; the simplex W[0..n) becomes the face that carries it.
RKH_DI void gjk_closest2(d3 a, d3 b, d3* W, int& n, d3& v) {
  const d3 ab = b - a;
  const double t = dot(mk3(0, 0, 0) - a, ab), den = dot(ab, ab);
  if (t <= 0.0 || den <= 0.0) { n = 1; W[0] = a; v = a; return; }
  if (t >= den) { n = 1; W[0] = b; v = b; return; }
  n = 2; W[0] = a; W[1] = b; v = gjk_foot(a, ab, t / den);
}

// The same on the simplex W[0..n), n = 1..3.
RKH_DI void gjk_closest3(d3* W, int& n, d3& v) {
  if (n == 1) {
    v = W[0];
    return;
  }
  if (n == 2) {
    gjk_closest2(W[0], W[1], W, n, v);
    return;
  }
  if (n == 3) {  // Ericson 5.1.5, query point = origin
    const d3 a = W[0], b = W[1], c = W[2];
    const d3 ab = b - a, ac = c - a, ap = mk3(0, 0, 0) - a;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { n = 1; W[0] = a; v = a; return; }
    const d3 bp = mk3(0, 0, 0) - b;
    const double d3_ = dot(ab, bp), d4 = dot(ac, bp);
    if (d3_ >= 0.0 && d4 <= d3_) { n = 1; W[0] = b; v = b; return; }
    const double vc = d1 * d4 - d3_ * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3_ <= 0.0) {
      const double t = d1 / (d1 - d3_);
      n = 2; W[0] = a; W[1] = b; v = gjk_foot(a, ab, t);
      return;
    }
    const d3 cp = mk3(0, 0, 0) - c;
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { n = 1; W[0] = c; v = c; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
      const double t = d2 / (d2 - d6);
      n = 2; W[0] = a; W[1] = c; v = gjk_foot(a, ac, t);
      return;
    }
    const double va = d3_ * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3_) >= 0.0 && (d5 - d6) >= 0.0) {
      const double t = (d4 - d3_) / ((d4 - d3_) + (d5 - d6));
      n = 2; W[0] = b; W[1] = c; v = gjk_foot(b, c - b, t);
      return;
    }
    // inside the face: the foot of the origin on its plane, along the normal (the barycentric sum a + s ab + t ac would
    // carry the rounding of |a| in every direction; the normal's direction is good to the rounding of the cross product)
    const d3 nrm = cross(ab, ac);
    const double nn = dot(nrm, nrm);
    if (nn <= kGjkFlat * kGjkFlat * dot(ab, ab) * dot(ac, ac)) {  // collinear to rounding, no plane: the longest edge is the hull
      const d3 bc = c - b;
      const double lab = dot(ab, ab), lac = dot(ac, ac), lbc = dot(bc, bc);
      gjk_closest2((lbc > lab && lbc > lac) ? b : a, (lab >= lac && lab >= lbc) ? b : c, W, n, v);
      return;
    }
    v = (dot(a, nrm) / nn) * nrm;
    return;
  }
}

// The same for n = 1..4.  Returns false when the origin is inside the tetrahedron (the sets intersect).
RKH_DI bool gjk_closest(d3* W, int& n, d3& v) {
  if (n < 4) {
    gjk_closest3(W, n, v);
    return true;
  }
  // n == 4: test the four faces the origin can be outside of (Ericson 5.1.6); keep the closest
  const d3 P[4] = {W[0], W[1], W[2], W[3]};
  const int F[4][4] = {{0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {1, 3, 2, 0}};  // face (i,j,k), opposite vertex l
  double best = INFINITY;
  d3 bestW[3];
  int bestN = 0;
  d3 bestV = mk3(0, 0, 0);
  bool outside_any = false;
#pragma unroll 1
  for (int f = 0; f < 4; ++f) {
    const d3 a = P[F[f][0]], b = P[F[f][1]], c = P[F[f][2]], dd = P[F[f][3]];
    const d3 nrm = cross(b - a, c - a);
    const double so = dot(mk3(0, 0, 0) - a, nrm), sd = dot(dd - a, nrm);
    // the origin is outside this face if it lies on the other side than the opposite vertex.  flat: that vertex lies in
    // the face's plane to rounding, so the sign of sd is noise and so is the side test -- take the face in any case
    const bool flat = sd * sd <= kGjkFlat * kGjkFlat * dot(nrm, nrm) * dot(dd - a, dd - a);
    if (flat || so * sd < 0.0) {
      outside_any = true;
      d3 T[3] = {a, b, c};
      int tn = 3;
      d3 tv;
      gjk_closest3(T, tn, tv);
      const double q = dot(tv, tv);
      if (q < best) {
        best = q;
        bestN = tn;
        bestV = tv;
        bestW[0] = T[0]; bestW[1] = T[1]; bestW[2] = T[2];
      }
    }
  }
  if (!outside_any) return false;  // inside all four faces
  n = bestN;
  for (int i = 0; i < bestN; ++i) W[i] = bestW[i];
  v = bestV;
  return true;
}

// distance between the two swept shapes (see the header comment)
RKH_DI double gjk_distance(const GjkShape& A, const GjkShape& B) {
  const double rsum = gjk_radius(A) + gjk_radius(B);
  d3 v = A.pos - B.pos;
  if (dot(v, v) == 0.0) v = mk3(1.0, 0.0, 0.0);
  d3 W[4];
  int n = 0;
#pragma unroll 1
  for (int it = 0;; ++it) {
    const d3 w = gjk_support(A, -v) - gjk_support(B, v);
    const double vv = dot(v, v), vw = dot(v, w);
    // certified: no point of A - B is closer to the origin than v by more than the tolerance (first pass: n == 0)
    if (n > 0 && (vv - vw) <= kGjkRelTol * vv + kGjkAbsTol * sqrt(vv * dot(w, w))) return sqrt(vv) - rsum;
    bool dup = false;
    for (int i = 0; i < n; ++i) dup = dup || (W[i].x == w.x && W[i].y == w.y && W[i].z == w.z);
    // not certified and no way on (repeated vertex, iteration cap): the lower bound itself, never |v|
    if (dup || it == kGjkMaxIter) return (vw > 0.0 ? vw / sqrt(vv) : 0.0) - rsum;
    W[n++] = w;
    if (!gjk_closest(W, n, v)) return -rsum - kGjkOverlap;
    if (dot(v, v) <= 1e-30) return -rsum - kGjkOverlap;  // the origin lies on the simplex
  }
}

// ---- the record of a pair: gjk_distance's value with a closest pair of points ------------------------------------------
// A search holds its witnesses: each simplex point is w_i = a_i - b_i with a_i, b_i support points of the two cores, and
// the closest point v of the simplex is a convex combination of the w_i; the same combination of the a_i (the b_i) is a
// point of core A (core B).  gjk_record runs gjk_distance's search -- the same support calls, the same exits in the same
// order, so dist is that function's value -- and keeps the a_i beside the w_i.
//   cores apart (every exit that returns ... - rsum): with lambda the barycentric coordinates of v in the final simplex,
//     pA = sum lambda_i a_i, pB = pA - v (v is perpendicular to its simplex to its own rounding; sum lambda_i b_i would
//     carry the rounding of |a| instead), n = -v / |v| (from A towards B; from the search's v, never from pB - pA, whose
//     direction at a gap of 1e-8 is good to 1e-8 only), point1 = pA + rA n, point2 = pB - rB n.
//   cores crossing (origin inside the tetrahedron, or on the simplex): lambda = the barycentric coordinates of the origin,
//     point1 = sum lambda_i a_i, point2 = point1 - sum lambda_i w_i (the same combination of the b_i): one common point
//     of the two cores, up to the conditioning of the simplex.  dist = -rsum - kGjkOverlap as in gjk_distance; there is no
//     penetration depth and none is invented.
// The combinations are taken about the first point, p_0 + sum_{i>0} lambda_i (p_i - p_0): the same point, and the
// rounding of lambda then scales with the simplex's edges, not with the distance of the shapes from the world's origin.
struct GjkRecord {
  d3 p1, p2;  // on shape A, on shape B (world frame)
  double dist;
};

// Barycentric coordinates of the closest point to the origin of the simplex W[0..n), n = 1..3, as gjk_closest leaves it:
// that point lies in the simplex's relative interior (a vertex: 1; an edge: its parameter; a face: Ericson 5.1.5's
// (va, vb, vc) / (va + vb + vc)).  Non-negative, sum 1.
RKH_DI void gjk_barycentric(const d3* W, int n, double* lam) {
  lam[0] = 1.0; lam[1] = 0.0; lam[2] = 0.0;
  if (n == 2) {
    const d3 ab = W[1] - W[0];
    const double t = dot(mk3(0, 0, 0) - W[0], ab), den = dot(ab, ab);
    const double s = (t <= 0.0 || den <= 0.0) ? 0.0 : (t >= den ? 1.0 : t / den);
    lam[0] = 1.0 - s; lam[1] = s;
  } else if (n == 3) {
    const d3 a = W[0], b = W[1], c = W[2];
    const d3 ab = b - a, ac = c - a, ap = mk3(0, 0, 0) - a, bp = mk3(0, 0, 0) - b, cp = mk3(0, 0, 0) - c;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap), d3_ = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
    double va = d3_ * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3_ * d2;
    va = va > 0.0 ? va : 0.0; vb = vb > 0.0 ? vb : 0.0; vc = vc > 0.0 ? vc : 0.0;
    const double s = va + vb + vc;
    if (s > 0.0) { lam[0] = va / s; lam[1] = vb / s; lam[2] = vc / s; }
  }
}

// The same for the origin inside the tetrahedron W[0..4) (gjk_closest returned false, so no face of it is flat): ratios
// of signed volumes, made non-negative and normalised.
RKH_DI void gjk_barycentric4(const d3* W, double* lam) {
  const double V0 = dot(W[1], cross(W[2], W[3])), V1 = -dot(W[0], cross(W[2], W[3]));
  const double V2 = dot(W[0], cross(W[1], W[3])), V3 = -dot(W[0], cross(W[1], W[2]));
  const double V = (V0 + V1) + (V2 + V3);  // the tetrahedron's own signed volume (x 6)
  const double sg = V < 0.0 ? -1.0 : 1.0;
  double l[4] = {sg * V0, sg * V1, sg * V2, sg * V3};
  double s = 0.0;
  for (int i = 0; i < 4; ++i) { l[i] = l[i] > 0.0 ? l[i] : 0.0; s += l[i]; }
  for (int i = 0; i < 4; ++i) lam[i] = s > 0.0 ? l[i] / s : (i == 0 ? 1.0 : 0.0);
}

// sum lambda_i P_i, about P_0
RKH_DI d3 gjk_combine(const d3* P, const double* lam, int n) {
  d3 p = P[0];
  for (int i = 1; i < n; ++i) p = p + lam[i] * (P[i] - P[0]);
  return p;
}

RKH_DI GjkRecord gjk_record_apart(const d3* W, const d3* S, int n, d3 v, double dist, double rA, double rB) {
  double lam[3];
  gjk_barycentric(W, n, lam);
  const d3 pA = gjk_combine(S, lam, n);
  const d3 pB = pA - v;
  const double len = sqrt(dot(v, v));
  const d3 nrm = mk3(-v.x / len, -v.y / len, -v.z / len);
  GjkRecord r;
  r.p1 = pA + rA * nrm;
  r.p2 = pB - rB * nrm;
  r.dist = dist;
  return r;
}

RKH_DI GjkRecord gjk_record_crossing(const d3* W, const d3* S, const double* lam, int n, double rsum) {
  GjkRecord r;
  r.p1 = gjk_combine(S, lam, n);
  r.p2 = r.p1 - gjk_combine(W, lam, n);
  r.dist = -rsum - kGjkOverlap;
  return r;
}

RKH_DI GjkRecord gjk_record(const GjkShape& A, const GjkShape& B) {
  const double rA = gjk_radius(A), rB = gjk_radius(B);
  const double rsum = rA + rB;
  d3 v = A.pos - B.pos;
  if (dot(v, v) == 0.0) v = mk3(1.0, 0.0, 0.0);
  d3 W[4], S[4];  // S[i]: A's support point of simplex point W[i]
  int n = 0;
#pragma unroll 1
  for (int it = 0;; ++it) {
    const d3 sa = gjk_support(A, -v);
    const d3 w = sa - gjk_support(B, v);
    const double vv = dot(v, v), vw = dot(v, w);
    if (n > 0 && (vv - vw) <= kGjkRelTol * vv + kGjkAbsTol * sqrt(vv * dot(w, w))) return gjk_record_apart(W, S, n, v, sqrt(vv) - rsum, rA, rB);
    bool dup = false;
    for (int i = 0; i < n; ++i) dup = dup || (W[i].x == w.x && W[i].y == w.y && W[i].z == w.z);
    if (dup || it == kGjkMaxIter) return gjk_record_apart(W, S, n, v, (vw > 0.0 ? vw / sqrt(vv) : 0.0) - rsum, rA, rB);
    W[n] = w;
    S[n] = sa;
    ++n;
    d3 W0[4], S0[4];
    const int n0 = n;
    for (int i = 0; i < n0; ++i) { W0[i] = W[i]; S0[i] = S[i]; }
    if (!gjk_closest(W, n, v)) {  // W is untouched
      double lam[4];
      gjk_barycentric4(W, lam);
      return gjk_record_crossing(W, S, lam, 4, rsum);
    }
    // gjk_closest moves and drops simplex points and computes none; no two are equal (dup above), so each survivor names
    // the support point that came with it
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n0; ++j)
        if (W[i].x == W0[j].x && W[i].y == W0[j].y && W[i].z == W0[j].z) S[i] = S0[j];
    if (dot(v, v) <= 1e-30) {  // the origin lies on the simplex
      double lam[3];
      gjk_barycentric(W, n, lam);
      return gjk_record_crossing(W, S, lam, n, rsum);
    }
  }
}

}  // namespace rkh
