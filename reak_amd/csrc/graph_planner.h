// graph_planner.h -- host rules shared by the drivers of the graph planners (rrtstar.hip, prm.hip, birrt.hip): one
// definition of each restated reference function, and the part of a planner handle that is the same for all of them.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "graph_batch.h"

namespace rkh {

constexpr uint32_t NIL = 0xFFFFFFFFu;

inline double euclid(const double* a, const double* b, int D) {  // vect_distance_metrics.hpp:126-137
  double r = 0.0;
  for (int i = 0; i < D; ++i) {
    const double d = a[i] - b[i];
    r += d * d;
  }
  return std::sqrt(r);
}

inline size_t highest_set_bit(size_t N) {  // math::highest_set_bit (core/base/misc_math.hpp:50-59): integer log2
  size_t temp = 0;
  for (size_t shift = sizeof(size_t) * 4; (shift && (N != 1)); shift >>= 1) {
    if (N >> shift) {
      temp |= shift;
      N >>= shift;
    }
  }
  return temp;
}

// star_neighborhood::operator() (ctrl/graph_alg/neighborhood_functors.hpp:95-102) for a graph of N vertices
inline void star_neighbourhood(size_t N, double gamma, int D, uint32_t* k, double* radius) {
  const size_t log_N = highest_set_bit(N) + 1;
  *k = uint32_t(4 * log_N);
  *radius = gamma * std::pow(log_N / double(N), 1.0 / double(D));
}

// the largest k star_neighbourhood asks for while a graph grows to max_vertices (+ start and goal)
inline uint32_t star_kmax(const std::vector<uint32_t>& max_vertices) {
  uint32_t max_v = 0;
  for (uint32_t m : max_vertices) max_v = std::max(max_v, m);
  return uint32_t(4 * (highest_set_bit(size_t(max_v) + 2) + 1));
}

// boost::uniform_01 on a 32-bit engine; word() is the engine's next output (std::mt19937, or PRM's replay window)
template <class Words>
double uniform_01(Words& word) {
  for (;;) {
    const double r = double(uint32_t(word())) * (1.0 / 4294967296.0);
    if (r < 1.0) return r;
  }
}

// hyperbox_topology::random_point (hyperbox_topology.hpp:97-103)
template <class Words>
void hyperbox_point(Words& word, const double* lower, const double* upper, int D, double* out) {
  for (int d = 0; d < D; ++d) out[d] = lower[d] + uniform_01(word) * (upper[d] - lower[d]);
}

template <class T>
void copy_out(T* dst, const std::vector<T>& src) {  // the getters: a null destination is an array the caller skips
  if (dst) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}

// What every planner handle holds: the device batch, the dimension of the space and its sampling box.
struct GraphHandle {
  GraphBatch gb;
  int D = 0;
  uint32_t P = 0;  // problems
  double lower[RKH_MAX_DOF], upper[RKH_MAX_DOF];

  // qs != nullptr: quasi-static free space (vertices = joint positions); dyn != nullptr: steerable dynamic free space
  // (vertices = states (q, qd), D = 2 n_dof; edges are RK4 propagations).  Every problem owns `slots` device trees
  // (slot = slots * problem + tree) with room for its max_vertices + 2 rows.
  rkh_status init(rkh_scene* scene, const rkh_qs_space* qs, const rkh_dyn_space* dyn,
                  const std::vector<uint32_t>& max_vertices, uint32_t slots, uint32_t kmax) {
    D = qs ? qs->n_dof : 2 * dyn->n_dof;
    P = uint32_t(max_vertices.size());
    for (int d = 0; d < D; ++d) {
      lower[d] = qs ? qs->lower[d] : dyn->lower[d];
      upper[d] = qs ? qs->upper[d] : dyn->upper[d];
    }
    std::vector<uint64_t> caps(size_t(slots) * P);
    for (size_t s = 0; s < caps.size(); ++s) caps[s] = uint64_t(max_vertices[s / slots]) + 2;
    return qs ? gb.init(scene, qs, uint32_t(caps.size()), caps.data(), kmax)
              : gb.init_dynamic(scene, dyn, uint32_t(caps.size()), caps.data(), kmax);
  }

  // the initial vertex rows: device step r appends row(r, slot) to every slot
  template <class Row>
  rkh_status append_initial_rows(int steps, Row row) {
    for (int r = 0; r < steps; ++r) {
      gb.begin();
      for (uint32_t s = 0; s < gb.P; ++s) {
        const rkh_status st = gb.cmd_append(s, row(r, s));
        if (st != RKH_OK) return st;
      }
      const rkh_status st = gb.run();
      if (st != RKH_OK) return st;
    }
    return RKH_OK;
  }
};

}  // namespace rkh
