// prox_record_ref_2d.cpp -- reference side of the planar proximity-record tests: every finder's proximity_record_2D and
// the min_i that proxy_query_pair_2D::findMinimumDistance leaves, from the CPU oracle's closed forms
// (oracle/reak_planar.hpp fills mPoint1 / mPoint2 in all six, but the oracle's C entry points return distances only).
//
// Input: the caller's rkh_shape array and the planar chain frames [B][n_frames][4] (position, rotation as (cos, sin)).
// Taking the frames instead of a state keeps this independent of the oracle's KteChain, which does not know
// prismatic_joint_2D: the frames come from tests/kte_ref_planar.py (revolute chains: also from orc_fk).
//
// Built at test time as a shared library:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I oracle -I include tests/cpp/prox_record_ref_2d.cpp
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

#include "reak_planar.hpp"

using namespace oracle;

namespace {
struct Env2 {
  std::vector<rkh_shape> shapes;
  std::vector<int> robot, env;
  std::vector<ProxFinder2> finders;
  Env2(const rkh_shape* s, int n) : shapes(s, s + n) {
    for (int i = 0; i < n; ++i) (shapes[i].anchor >= 0 ? robot : env).push_back(i);
    createProxFinderList2D(shapes, robot, env, finders);
  }
  // pose_2D::getGlobalPose of every shape (ProxyEnv::resolve2)
  void resolve(const double* frames, std::vector<ShapeG2>& g) const {
    g.resize(shapes.size());
    for (std::size_t i = 0; i < shapes.size(); ++i) {
      const rkh_shape& s = shapes[i];
      g[i].kind = s.kind;
      for (int k = 0; k < 2; ++k) g[i].dims[k] = s.dims[k];
      const Pose2 local = to_pose2(s.pose);
      if (s.anchor >= 0) {
        const double* f = frames + 4 * std::size_t(s.anchor);
        Pose2 parent;
        parent.Position = V2(f[0], f[1]);
        parent.Rotation = Rot2(f[2], f[3]);
        g[i].g = global_pose2(&parent, local);
      } else {
        g[i].g = local;
      }
    }
  }
};
}  // namespace

extern "C" {

// number of finders of createProxFinderList for these shapes (robot model = anchored shapes, environment = the rest)
int prr2_num_finders(const rkh_shape* shapes, int n_shapes) { return int(Env2(shapes, n_shapes).finders.size()); }

// For each of B frame sets, every finder in finder order: (s1, s2) = indices into `shapes` in the finder's own order, the
// routine (11..16), the bounding-circle gap |c2 - c1| - r1 - r2 of proxy_query_model.cpp:176-180 / :196-200, and the
// record.  winner[b] = min_i after the loop of :163-187 replayed as the sequence it is (finder 0 always computed, finder
// i >= 1 skipped when its gap > min_dist, else it takes over on a strictly smaller distance), -1 without finders;
// margin[b] = the smallest |gap - min_dist| or (where the finder was computed) |dist - min_dist| any decision of that
// replay had, +inf with fewer than two finders: how far the replay was from going another way.
// Arrays: s1, s2, routine [nf]; gap, dist [B][nf]; p1, p2 [B][nf][2]; winner, margin [B].  Returns nf.
int prr2_records(const rkh_shape* shapes, int n_shapes, const double* frames, int n_frames, int B, int* s1, int* s2,
                 int* routine, double* gap, double* dist, double* p1, double* p2, int* winner, double* margin) {
  const Env2 env(shapes, n_shapes);
  const std::size_t nf = env.finders.size();
  for (std::size_t i = 0; i < nf; ++i) {
    s1[i] = env.finders[i].s1;
    s2[i] = env.finders[i].s2;
    routine[i] = env.finders[i].routine;
  }
  std::vector<ShapeG2> g;
  for (int b = 0; b < B; ++b) {
    env.resolve(frames + std::size_t(b) * n_frames * 4, g);
    std::size_t min_i = 0;
    double min_dist = 0.0, mg = std::numeric_limits<double>::infinity();
    for (std::size_t i = 0; i < nf; ++i) {
      const ProxFinder2& f = env.finders[i];
      const V2 c1 = g[f.s1].g.transformToParent(V2(0.0, 0.0));
      const V2 c2 = g[f.s2].g.transformToParent(V2(0.0, 0.0));
      const double gp = norm_2(c2 - c1) - g[f.s1].getBoundingRadius() - g[f.s2].getBoundingRadius();
      const ProxRecord2 r = computeProximity2D(f, g);
      const std::size_t at = std::size_t(b) * nf + i;
      gap[at] = gp;
      dist[at] = r.mDistance;
      for (int k = 0; k < 2; ++k) {
        p1[2 * at + k] = r.mPoint1[k];
        p2[2 * at + k] = r.mPoint2[k];
      }
      if (i == 0) {
        min_dist = r.mDistance;
        continue;
      }
      mg = std::fmin(mg, std::fabs(gp - min_dist));
      if (gp > min_dist) continue;
      mg = std::fmin(mg, std::fabs(r.mDistance - min_dist));
      if (r.mDistance < min_dist) {
        min_i = i;
        min_dist = r.mDistance;
      }
    }
    winner[b] = nf ? int(min_i) : -1;
    margin[b] = mg;
  }
  return int(nf);
}

// One pair of world-anchored shapes already in the finder's (shape1, shape2) order, by routine number: the record
// [p1 (2), p2 (2), distance], for B pairs.
void prr2_pair_records(const rkh_shape* a, const rkh_shape* b, int routine, int B, double* out) {
  std::vector<ShapeG2> g(2);
  for (int i = 0; i < B; ++i) {
    const rkh_shape* sh[2] = {a + i, b + i};
    for (int k = 0; k < 2; ++k) {
      g[k].kind = sh[k]->kind;
      g[k].g = to_pose2(sh[k]->pose);
      for (int d = 0; d < 2; ++d) g[k].dims[d] = sh[k]->dims[d];
    }
    const ProxRecord2 r = computeProximity2D(ProxFinder2{routine, 0, 1}, g);
    for (int k = 0; k < 2; ++k) {
      out[5 * i + k] = r.mPoint1[k];
      out[5 * i + 2 + k] = r.mPoint2[k];
    }
    out[5 * i + 4] = r.mDistance;
  }
}

}  // extern "C"
