// epa_device.h -- penetration depth and contact normal of support-map pairs whose cores cross: the Expanding Polytope
// Algorithm (van den Bergen, "Proximity queries and penetration depth computation on 3D game objects", 2001) on the
// Minkowski difference D = A - B of the two cores, started from the simplex the GJK search of gjk_device.h ends with.
//
// gjk_depth_record / gjk_depth_distance run gjk_record's search -- the same support calls, the same exits in the same
// order -- and on every exit with the cores apart return what gjk_record / gjk_distance return, bit for bit.  On the two
// crossing exits (the origin inside the tetrahedron; the origin on a simplex of fewer than 4 points, exact touching
// among them) they go on where gjk_record stops:
//   * start-up: a simplex of 1, 2 or 3 points grows into a tetrahedron that holds the origin (inside or on its
//     boundary) -- one point: the farthest support point along +-x, +-y, +-z; two: the support point highest above the
//     line along four directions across it; three: the higher of the support points along +- the triangle's normal.
//     Where the best candidate is no taller than kGjkFlat times the simplex's edge, D is flat (both cores in one plane
//     or line): depth 0, n = the flat's unit normal as the start-up leaves it, points = gjk_record_crossing's common
//     point stepped out by the radii;
//   * the polytope: at most kEpaMaxVerts vertices, each with A's support point beside it (as S[] in gjk_record), and
//     triangular faces with their unit outward normal and plane distance.  The closest face is the one of least plane
//     distance d (the origin is in the polytope, so its foot lies in that face); with w the support point of D along the
//     face's normal n,  d <= depth <= n.w.  d is returned once certified by that bound,
//         n.w - d  <=  kGjkRelTol d + kGjkAbsTol |w|
//     (gjk_distance's rule).  Otherwise w joins the polytope: the faces that see it (n_f.w - d_f above the rounding
//     kGjkAbsTol |w|, so faces coplanar with w stay) leave, and each edge between a face that leaves and one that stays
//     gets a new face to w in the leaving face's winding, which keeps every normal outward without a look at the origin
//     (it may lie ON the boundary);
//   * no way on -- w is a vertex already, or the vertex, face or horizon-edge cap is reached: the result is the UPPER
//     bound n.w of the depth, so the distance errs below, never above, as gjk_distance's does;
//   * result: depth, n = the closest face's outward normal (from shape 1 towards shape 2, the sign of gjk_record_apart's
//     nrm: moving shape 2 by depth n brings the cores to touching), dist = -(rA + rB + depth) - kGjkOverlap,
//     point1 = sum lambda_i a_i + rA n, point2 = point1 - (depth + rA + rB) n, with lambda the barycentric coordinates of
//     the origin's foot d n on the closest face, combined about the first point (gjk_combine).
// Every pair the finder cascade hands to the support-map query has polytope cores (point, segment, 8 corners, vertex
// set: proximity_device.h's pair_routine), so D is a polytope and the expansion ends by itself; the caps bound every loop
// all the same.
//
// Thin facets.  A face's normal is the cross product of the two edges that meet OPPOSITE its longest edge: all three
// pairs of edges give the same vector, twice the area, with a rounding of a few ulps of |e1| |e2|, and that pair has
// the smallest product, hence the smallest relative error (for a needle the short edge and a long one, never the two
// long ones).  The plane distance is n.(the vertex the two edges meet at), good to the rounding of that vertex.  A face
// whose area is rounding noise (its height below kGjkFlat times its edge) carries no plane: it is never the closest face
// and never leaves, an edge of the polytope drawn as a face.  Whatever a thin face's normal is worth, the exit certifies
// its own result: n is a unit vector, so n.w is the width of D along n and bounds the depth from above.
//
// The cap.  On the host build (tests/cpp/epa_record_host.cpp) over the families of tests/penetration_ref.py -- 300
// shallow and 60 deep mesh pairs of 4-32 vertices, 60 mesh / sphere, capped cylinder, box pairs, the hand-built cases --
// the largest polytope had 27 vertices (23 expansions of the tetrahedron; a pair of 12 and 23 vertices 0.2 deep; seven
// other draws of the deep family stayed at 19 to 23); kEpaMaxVerts = 64 is 2.4 times that.  The closed surface of V
// vertices has 2V - 4 faces (kEpaMaxFaces = 2 kEpaMaxVerts: the two 64-bit masks of the leaving faces) and a horizon
// of at most V edges.  Private arrays per lane: vertices with their support points 48 V, faces (normal, distance, three
// indices: 40 bytes) 40 x 2V, horizon 2V bytes = 130 V = 8320 bytes.
#pragma once
#include "gjk_device.h"

#ifndef RKH_EPA_NOTE  // the host build counts polytope vertices through this hook
#define RKH_EPA_NOTE(n_verts)
#endif

namespace rkh {

constexpr int kEpaMaxVerts = 64;
constexpr int kEpaMaxFaces = 2 * kEpaMaxVerts;
constexpr int kEpaMaxHorizon = kEpaMaxVerts;

struct GjkDepthRecord {
  d3 p1, p2;  // on shape A, on shape B (world frame)
  d3 nrm;     // unit, from A towards B
  double dist;
};

// Unit normal of the triangle (a, b, c) in its winding and its plane's distance from the origin (see "Thin facets").
// false: the triangle has no plane (n = 0, d = +inf).
RKH_DI bool epa_plane(d3 a, d3 b, d3 c, d3& n, double& d) {
  const d3 ab = b - a, bc = c - b, ca = a - c;
  const double lab = dot(ab, ab), lbc = dot(bc, bc), lca = dot(ca, ca);
  d3 e1, e2, apex;
  double l1, l2;
  if (lbc >= lab && lbc >= lca) { apex = a; e1 = ab; e2 = -ca; l1 = lab; l2 = lca; }
  else if (lca >= lab) { apex = b; e1 = bc; e2 = -ab; l1 = lbc; l2 = lab; }
  else { apex = c; e1 = ca; e2 = -bc; l1 = lca; l2 = lbc; }
  const d3 nrm = cross(e1, e2);
  const double nn = dot(nrm, nrm);
  if (!(nn > kGjkFlat * kGjkFlat * l1 * l2)) {
    n = mk3(0.0, 0.0, 0.0);
    d = INFINITY;
    return false;
  }
  const double len = sqrt(nn);
  n = mk3(nrm.x / len, nrm.y / len, nrm.z / len);
  d = dot(n, apex);
  return true;
}

// support point of D = A - B along dir, and A's own
RKH_DI d3 epa_support(const GjkShape& A, const GjkShape& B, d3 dir, d3& sa) {
  sa = gjk_support(A, dir);
  return sa - gjk_support(B, -dir);
}

RKH_DI d3 epa_unit(d3 v) {
  const double len = sqrt(dot(v, v));
  return mk3(v.x / len, v.y / len, v.z / len);
}

struct EpaVert {
  d3 w, a;  // a vertex of the polytope (a point of D), and A's support point of it
};
struct EpaFace {
  d3 n;      // unit outward normal (0: no plane)
  double d;  // the plane's distance from the origin (+inf: no plane)
  unsigned char i, j, k;
};

RKH_DI bool epa_has_edge(const EpaFace& g, unsigned char a, unsigned char b) {  // the directed edge (a, b), in g's winding
  return (g.i == a && g.j == b) || (g.j == a && g.k == b) || (g.k == a && g.i == b);
}

// The crossing exits of gjk_depth_record: the simplex W[0..n) of D with A's support points S[0..n), the origin in its
// hull; `common` = gjk_record_crossing's record of it.  See the header comment.
RKH_DI GjkDepthRecord epa_record(const GjkShape& A, const GjkShape& B, const d3* W, const d3* S, int n, const GjkRecord& common,
                                 double rA, double rB) {
  EpaVert V[kEpaMaxVerts];
  EpaFace F[kEpaMaxFaces];
  unsigned char H[kEpaMaxHorizon][2];
  int nv = n;
  for (int i = 0; i < n; ++i) { V[i].w = W[i]; V[i].a = S[i]; }

  // ---- start-up: a tetrahedron around the origin, or a flat D
  bool flat = false;
  d3 flat_n = mk3(1.0, 0.0, 0.0);
  if (nv == 1) {
    double best = 0.0;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
      const double sg = (k & 1) ? -1.0 : 1.0;
      d3 sa;
      const d3 w = epa_support(A, B, mk3(k < 2 ? sg : 0.0, (k >= 2 && k < 4) ? sg : 0.0, k >= 4 ? sg : 0.0), sa);
      const d3 q = w - V[0].w;
      const double h = dot(q, q);
      if (h > best) { best = h; V[1].w = w; V[1].a = sa; }
    }
    if (best > 0.0) nv = 2;
    else flat = true;  // D is one point
  }
  if (!flat && nv == 2) {
    const d3 u = V[1].w - V[0].w;
    const double uu = dot(u, u);
    const double ax = fabs(u.x), ay = fabs(u.y), az = fabs(u.z);
    const d3 least = (ax <= ay && ax <= az) ? mk3(1.0, 0.0, 0.0) : (ay <= az ? mk3(0.0, 1.0, 0.0) : mk3(0.0, 0.0, 1.0));
    const d3 d1 = epa_unit(cross(u, least)), d2 = epa_unit(cross(u, d1));
    flat_n = d1;
    double best = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const d3 dir = k < 2 ? d1 : d2;
      d3 sa;
      const d3 w = epa_support(A, B, (k & 1) ? -dir : dir, sa);
      const d3 q = w - V[0].w;
      const d3 qp = q - (dot(q, u) / uu) * u;
      const double h = dot(qp, qp);
      if (h > best) { best = h; V[2].w = w; V[2].a = sa; }
    }
    if (best > kGjkFlat * kGjkFlat * uu) nv = 3;
    else flat = true;  // D lies in a line
  }
  if (!flat && nv == 3) {
    d3 nt;
    double dt;
    if (epa_plane(V[0].w, V[1].w, V[2].w, nt, dt)) {
      flat_n = nt;
      const d3 e1 = V[1].w - V[0].w, e2 = V[2].w - V[0].w, e3 = V[2].w - V[1].w;
      double edge = dot(e1, e1);
      edge = dot(e2, e2) > edge ? dot(e2, e2) : edge;
      edge = dot(e3, e3) > edge ? dot(e3, e3) : edge;
      double best = 0.0;
#pragma unroll 1
      for (int k = 0; k < 2; ++k) {
        d3 sa;
        const d3 w = epa_support(A, B, k ? -nt : nt, sa);
        const double h = fabs(dot(nt, w - V[0].w));
        if (h > best) { best = h; V[3].w = w; V[3].a = sa; }
      }
      if (best * best > kGjkFlat * kGjkFlat * edge) nv = 4;
      else flat = true;  // D lies in a plane
    } else {
      flat = true;
    }
  }
  GjkDepthRecord r;
  if (flat) {
    RKH_EPA_NOTE(nv);
    r.nrm = flat_n;
    r.p1 = common.p1 + rA * flat_n;
    r.p2 = common.p2 - rB * flat_n;
    r.dist = -((rA + rB) + 0.0) - kGjkOverlap;
    return r;
  }

  // ---- the tetrahedron's faces, each wound so that its normal points away from the fourth vertex
  int nf = 4;
#pragma unroll 1
  for (int f = 0; f < 4; ++f) {
    EpaFace t;  // faces (0 1 2), (0 2 3), (0 3 1), (1 3 2) against vertices 3, 1, 2, 0
    t.i = f == 3 ? 1 : 0;
    t.j = f == 0 ? 1 : (f == 1 ? 2 : 3);
    t.k = f == 0 ? 2 : (f == 1 ? 3 : (f == 2 ? 1 : 2));
    const int opp = f == 0 ? 3 : (f == 1 ? 1 : (f == 2 ? 2 : 0));
    epa_plane(V[t.i].w, V[t.j].w, V[t.k].w, t.n, t.d);
    if (dot(t.n, V[opp].w) - t.d > 0.0) {
      const unsigned char s = t.j; t.j = t.k; t.k = s;
      t.n = -t.n;
      t.d = -t.d;
    }
    F[f] = t;
  }

  // ---- expansion
  int fb = 0;
  double depth = 0.0;
#pragma unroll 1
  for (;;) {
    fb = 0;
    double db = F[0].d;
    for (int f = 1; f < nf; ++f)
      if (F[f].d < db) { db = F[f].d; fb = f; }
    const d3 nb = F[fb].n;
    d3 sa;
    const d3 w = epa_support(A, B, nb, sa);
    const double hw = dot(nb, w), lw = sqrt(dot(w, w));
    depth = db;
    if (hw - db <= kGjkRelTol * fabs(db) + kGjkAbsTol * lw) break;  // certified
    depth = hw;  // from here on every exit is "no way on": the upper bound
    bool dup = false;
    for (int i = 0; i < nv; ++i) dup = dup || (V[i].w.x == w.x && V[i].w.y == w.y && V[i].w.z == w.z);
    if (dup || nv == kEpaMaxVerts) break;
    // the faces that see w (bit f of vis0 / vis1)
    unsigned long long vis0 = 0ull, vis1 = 0ull;
    int n_vis = 0;
    for (int f = 0; f < nf; ++f) {
      if (F[f].d < INFINITY && dot(F[f].n, w) - F[f].d > kGjkAbsTol * lw) {
        if (f < 64) vis0 |= 1ull << f;
        else vis1 |= 1ull << (f - 64);
        ++n_vis;
      }
    }
    auto sees = [&](int f) { return ((f < 64 ? vis0 >> f : vis1 >> (f - 64)) & 1ull) != 0ull; };
    // the horizon: edges (a, b) of a leaving face whose neighbour across, the face with the edge (b, a), stays
    int nh = 0;
    bool full = false;
    for (int t = 0; t < 3 * nf && !full; ++t) {  // edge e of face f, t = 3 f + e
      const int f = t / 3, e = t - 3 * f;
      const EpaFace ff = F[f];
      const unsigned char a = e == 0 ? ff.i : (e == 1 ? ff.j : ff.k), b = e == 0 ? ff.j : (e == 1 ? ff.k : ff.i);
      bool leaves = false;
      for (int g = 0; g < nf; ++g) leaves = leaves || (epa_has_edge(F[g], b, a) && sees(g));
      if (!sees(f) || leaves) continue;
      if (nh == kEpaMaxHorizon) {
        full = true;
      } else {
        H[nh][0] = a; H[nh][1] = b;
        ++nh;
      }
    }
    if (full || nf - n_vis + nh > kEpaMaxFaces) break;
    // the leaving faces go (the last face takes the place of each, from the top down), the new ones follow
    for (int f = nf - 1; f >= 0; --f) {
      if (!sees(f)) continue;
      --nf;
      F[f] = F[nf];
    }
    V[nv].w = w;
    V[nv].a = sa;
    for (int h = 0; h < nh; ++h) {
      EpaFace t;
      t.i = H[h][0]; t.j = H[h][1]; t.k = (unsigned char)nv;
      epa_plane(V[t.i].w, V[t.j].w, w, t.n, t.d);
      F[nf] = t;
      ++nf;
    }
    ++nv;
  }
  RKH_EPA_NOTE(nv);

  // ---- the record: the origin's foot on the closest face.  A facet of D with more than three vertices is several
  // coplanar faces here, of equal distance to rounding, and the foot lies in one of them: among the faces no farther than
  // the certificate's tolerance, the one whose own foot is deepest inside its triangle (largest least barycentric coordinate)
  {
    const double dmax = F[fb].d + (kGjkRelTol * fabs(F[fb].d) + kGjkAbsTol * sqrt(dot(V[nv - 1].w, V[nv - 1].w)));
    double in_best = -INFINITY;
    for (int f = 0; f < nf; ++f) {
      const EpaFace ff = F[f];
      const d3 v0 = V[ff.i].w;
      const d3 p = ff.d * ff.n - v0, e0 = V[ff.j].w - v0, e1 = V[ff.k].w - v0;
      const double d00 = dot(e0, e0), d01 = dot(e0, e1), d11 = dot(e1, e1), d20 = dot(p, e0), d21 = dot(p, e1);
      const double den = d00 * d11 - d01 * d01;
      const double bv = (d11 * d20 - d01 * d21) / den, bw = (d00 * d21 - d01 * d20) / den, bu = (1.0 - bv) - bw;
      const double in = fmin(bu, fmin(bv, bw));
      if (ff.d <= dmax && in > in_best) { in_best = in; fb = f; }
    }
  }
  const EpaFace fc = F[fb];
  const d3 foot = fc.d * fc.n;
  const d3 T[3] = {V[fc.i].w - foot, V[fc.j].w - foot, V[fc.k].w - foot};
  const d3 P[3] = {V[fc.i].a, V[fc.j].a, V[fc.k].a};
  double lam[3];
  gjk_barycentric(T, 3, lam);
  depth = depth > 0.0 ? depth : 0.0;
  r.nrm = fc.n;
  r.p1 = gjk_combine(P, lam, 3) + rA * fc.n;
  r.p2 = r.p1 - ((depth + rA) + rB) * fc.n;
  r.dist = -((rA + rB) + depth) - kGjkOverlap;
  return r;
}

RKH_DI GjkDepthRecord gjk_depth_apart(const GjkRecord& g, d3 v) {
  const double len = sqrt(dot(v, v));
  GjkDepthRecord r;
  r.p1 = g.p1;
  r.p2 = g.p2;
  r.dist = g.dist;
  r.nrm = mk3(-v.x / len, -v.y / len, -v.z / len);  // gjk_record_apart's nrm
  return r;
}

// gjk_record with the depth and the normal (see the header comment)
RKH_DI GjkDepthRecord gjk_depth_record(const GjkShape& A, const GjkShape& B) {
  const double rA = gjk_radius(A), rB = gjk_radius(B);
  const double rsum = rA + rB;
  d3 v = A.pos - B.pos;
  if (dot(v, v) == 0.0) v = mk3(1.0, 0.0, 0.0);
  d3 W[4], S[4];
  double lam[4];  // of the origin in the simplex, at the crossing exits
  int n = 0;
#pragma unroll 1
  for (int it = 0;; ++it) {
    const d3 sa = gjk_support(A, -v);
    const d3 w = sa - gjk_support(B, v);
    const double vv = dot(v, v), vw = dot(v, w);
    if (n > 0 && (vv - vw) <= kGjkRelTol * vv + kGjkAbsTol * sqrt(vv * dot(w, w)))
      return gjk_depth_apart(gjk_record_apart(W, S, n, v, sqrt(vv) - rsum, rA, rB), v);
    bool dup = false;
    for (int i = 0; i < n; ++i) dup = dup || (W[i].x == w.x && W[i].y == w.y && W[i].z == w.z);
    if (dup || it == kGjkMaxIter)
      return gjk_depth_apart(gjk_record_apart(W, S, n, v, (vw > 0.0 ? vw / sqrt(vv) : 0.0) - rsum, rA, rB), v);
    W[n] = w;
    S[n] = sa;
    ++n;
    d3 W0[4], S0[4];
    const int n0 = n;
    for (int i = 0; i < n0; ++i) { W0[i] = W[i]; S0[i] = S[i]; }
    if (!gjk_closest(W, n, v)) {  // the origin is inside the tetrahedron (W is untouched)
      gjk_barycentric4(W, lam);
      break;
    }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n0; ++j)
        if (W[i].x == W0[j].x && W[i].y == W0[j].y && W[i].z == W0[j].z) S[i] = S0[j];
    if (dot(v, v) <= 1e-30) {  // the origin lies on the simplex
      gjk_barycentric(W, n, lam);
      break;
    }
  }
  return epa_record(A, B, W, S, n, gjk_record_crossing(W, S, lam, n, rsum), rA, rB);
}

// its distance alone: the record's, so the two agree bit for bit
RKH_DI double gjk_depth_distance(const GjkShape& A, const GjkShape& B) { return gjk_depth_record(A, B).dist; }

}  // namespace rkh
