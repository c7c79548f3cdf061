// prox_record_ref.cpp -- reference side of the proximity-record tests: every finder's proximity_record_3D and the winner
// of proxy_query_pair_3D::findMinimumDistance, from the CPU oracle's closed forms (oracle/reak_proximity.hpp fills
// mPoint1 / mPoint2 in all eleven, but the oracle's C entry points return distances only).
//
// Input: the caller's rkh_shape array and the chain frames [B][n_frames][7] (position, quaternion).  Taking the frames
// instead of a state keeps this independent of the oracle's KteChain, which does not know prismatic joints: their frames
// come from tests/kte_ref.py, all others from orc_fk.
//
// Built at test time as a shared library:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I oracle -I include tests/cpp/prox_record_ref.cpp
#include <cstddef>
#include <vector>

#include "reak_proximity.hpp"

using namespace oracle;

namespace {
void resolve(const ProxyEnv& env, const double* frames, std::vector<ShapeG>& g) {
  g.resize(env.shapes.size());
  for (std::size_t i = 0; i < env.shapes.size(); ++i) {
    const rkh_shape& s = env.shapes[i];
    g[i].kind = s.kind;
    for (int k = 0; k < 3; ++k) g[i].dims[k] = s.dims[k];
    const Pose local = to_pose(s.pose);
    if (s.anchor >= 0) {  // pose_3D::getGlobalPose (ProxyEnv::resolve)
      const double* f = frames + 7 * std::size_t(s.anchor);
      Pose parent;
      parent.Position = V3(f[0], f[1], f[2]);
      parent.Q = Quat(f[3], f[4], f[5], f[6]);
      g[i].g = global_pose(&parent, local);
    } else {
      g[i].g = local;
    }
  }
}
}  // namespace

extern "C" {

// number of finders of createProxFinderList for these shapes (robot model = anchored shapes, environment = the rest)
int prr_num_finders(const rkh_shape* shapes, int n_shapes) { return int(ProxyEnv(shapes, n_shapes).finders.size()); }

// For each of B frame sets, every finder in finder order: (s1, s2) = indices into `shapes` in the finder's own order,
// the routine (1..11), the bounding-sphere gap |c2 - c1| - r1 - r2 of proxy_query_model.cpp:386-389 / :407-410, and
// the record.  winner[b] = min_i of findMinimumDistance's loop (:376-400, with its skip), -1 without finders.
// Arrays: s1, s2, routine [nf]; gap, dist [B][nf]; p1, p2 [B][nf][3]; winner [B].  Returns nf.
int prr_records(const rkh_shape* shapes, int n_shapes, const double* frames, int n_frames, int B, int* s1, int* s2,
                int* routine, double* gap, double* dist, double* p1, double* p2, int* winner) {
  const ProxyEnv env(shapes, n_shapes);
  const std::size_t nf = env.finders.size();
  for (std::size_t i = 0; i < nf; ++i) {
    s1[i] = env.finders[i].s1;
    s2[i] = env.finders[i].s2;
    routine[i] = env.finders[i].routine;
  }
  std::vector<ShapeG> g;
  for (int b = 0; b < B; ++b) {
    resolve(env, frames + std::size_t(b) * n_frames * 7, g);
    std::size_t min_i = 0;
    double min_dist = 0.0;
    for (std::size_t i = 0; i < nf; ++i) {
      const ProxFinder& f = env.finders[i];
      const V3 c1 = g[f.s1].g.transformToParent(V3(0, 0, 0));
      const V3 c2 = g[f.s2].g.transformToParent(V3(0, 0, 0));
      const double gp = norm_2(c2 - c1) - g[f.s1].getBoundingRadius() - g[f.s2].getBoundingRadius();
      const ProxRecord r = computeProximity(f, g);
      const std::size_t at = std::size_t(b) * nf + i;
      gap[at] = gp;
      dist[at] = r.mDistance;
      for (int k = 0; k < 3; ++k) {
        p1[3 * at + k] = r.mPoint1[k];
        p2[3 * at + k] = r.mPoint2[k];
      }
      if (i == 0) {
        min_dist = r.mDistance;
      } else if (!(gp > min_dist) && min_dist > r.mDistance) {
        min_i = i;
        min_dist = r.mDistance;
      }
    }
    winner[b] = nf ? int(min_i) : -1;
  }
  return int(nf);
}

// One pair of world-anchored shapes already in the finder's (shape1, shape2) order, by routine number: the record
// [p1 (3), p2 (3), distance], for B pairs.
void prr_pair_records(const rkh_shape* a, const rkh_shape* b, int routine, int B, double* out) {
  std::vector<ShapeG> g(2);
  for (int i = 0; i < B; ++i) {
    const rkh_shape* sh[2] = {a + i, b + i};
    for (int k = 0; k < 2; ++k) {
      g[k].kind = sh[k]->kind;
      g[k].g = to_pose(sh[k]->pose);
      for (int d = 0; d < 3; ++d) g[k].dims[d] = sh[k]->dims[d];
    }
    const ProxRecord r = computeProximity(ProxFinder{routine, 0, 1}, g);
    for (int k = 0; k < 3; ++k) {
      out[7 * i + k] = r.mPoint1[k];
      out[7 * i + 3 + k] = r.mPoint2[k];
    }
    out[7 * i + 6] = r.mDistance;
  }
}

}  // extern "C"
