// svp_device.h -- the order-1 rate-limited joint space with sustained-velocity-pulse (SVP) profiles, as functions of scalars.
//
// What it restates (reference paths relative to src/ReaK/ctrl/; semantics only):
//   svp_Ndof_compute_min_delta_time     interpolation/sustained_velocity_pulse_Ndof_detail.cpp:229-285  -> svp_joint_min_time
//   svp_Ndof_compute_peak_velocity      ..._detail.cpp:401-516                                          -> svp_joint_peak
//   svp_Ndof_compute_interpolated_values ..._detail.cpp:52-106                                          -> svp_joint_point
//   svp_compute_Ndof_interpolation_data_impl with delta_time = 0, ..._detail.hpp:163-201                 -> svp_reach
//   svp_Ndof_is_in_bounds               interpolation/sustained_velocity_pulse_Ndof.hpp:132-174         -> svp_in_bounds
//
// A point is (p0, v0, p1, v1, ...) in space coordinates (Ndof_rl_space<., 1>): p = q / speed_limit, v = qd / accel_limit.
// Positions move at rate v / vm with vm = speed_limit / accel_limit and |v| <= vm; velocities move at rate +-1 or 0, so
// all times below are travel times.  Where the reference throws optim::infeasible_problem these functions return false.
//
// Only +, -, *, /, sqrt, fabs and comparisons in fp64; every expression is written with its grouping so that, with
// contraction off, a host compiler, the device compiler and the Python twin (tests/svp_ref.py) round alike.  Nothing here
// uses a device builtin: with the stand-in for <hip/hip_runtime.h> a host compiler reads this header as it is
// (tests/cpp/svp_host.cpp), and rkh_svp_in_bounds runs it on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "steer_edge.h"  // RKH_HD, hyperbox_out

namespace rkh {

constexpr int kSvpMaxDof = 12;  // = kMaxDof (rkh_internal.h)

struct SvpDev {  // rkh_svp_space as the kernels take it (by value); limits of 0 already replaced by 1
  int32_t n;
  int32_t pad;
  double min_interval;
  double lower[kSvpMaxDof], upper[kSvpMaxDof];
  double speed[kSvpMaxDof], accel[kSvpMaxDof];
  double vm[kSvpMaxDof];  // speed / accel
};

// T - |vp - v0| - |v1 - vp|: the cruise time a peak velocity vp leaves in a profile of total time T
RKH_HD double svp_cruise_time(double vp, double v0, double v1, double T) { return (T - fabs(vp - v0)) - fabs(v1 - vp); }

// The "same point" shortcut every solver starts with.
RKH_HD bool svp_same_point(double p0, double p1, double v0, double v1, double vm) {
  return (fabs(p1 - p0) < 1e-6 * vm) && (fabs(v1 - v0) < 1e-6 * vm);
}

// Minimum travel time of one joint from (p0, v0) to (p1, v1), and the peak velocity of that profile.
RKH_HD bool svp_joint_min_time(double p0, double p1, double v0, double v1, double vm, double* t, double* peak) {
  *t = 0.0;
  *peak = v0;
  if (svp_same_point(p0, p1, v0, v1, vm)) return true;
  *peak = 0.0;
  if ((fabs(v0) > vm) || (fabs(v1) > vm)) return false;
  const double s = (p0 > p1) ? -1.0 : 1.0;
  // a cruise at full speed towards p1
  double vp = s * vm;
  const double vpd = vp / vm;
  const double rest = ((p1 - p0) - (0.5 * fabs(vp - v1)) * (vpd + v1 / vm)) - (0.5 * fabs(vp - v0)) * (vpd + v0 / vm);
  if (rest * vp > 0.0) {
    *peak = vp;
    *t = (fabs(rest) + fabs(vp - v1)) + fabs(vp - v0);
    return true;
  }
  // no cruise: the peak lies beyond both end velocities in the direction of travel
  const double dist = vm * fabs(p1 - p0);
  vp = sqrt((dist + (0.5 * v0) * v0) + (0.5 * v1) * v1);
  if ((vp > s * v0) && (vp > s * v1)) {
    vp = vp * s;
    *peak = vp;
    *t = fabs(vp - v1) + fabs(vp - v0);
    return true;
  }
  // ... or short of both
  if (dist < 0.5 * (v0 * v0 + v1 * v1)) {
    vp = sqrt(((0.5 * v0) * v0 + (0.5 * v1) * v1) - dist);
    if ((vp < s * v0) && (vp < s * v1)) vp = vp * s;
    else vp = vp * -s;
    *peak = vp;
    *t = fabs(vp - v1) + fabs(vp - v0);
    return true;
  }
  return false;
}

// the guards every candidate of svp_joint_peak passes: within 1.001 vm, and a cruise time not below -1e-3 vm
RKH_HD bool svp_peak_guard(double r, double vp, double v0, double v1, double vm, double T) {
  return (fabs(r) < 1.001 * vm) && (svp_cruise_time(vp, v0, v1, T) >= -1e-3 * vm);
}

// Peak velocity with which the joint takes exactly T (>= its own minimum).  The candidates in the reference's order:
// beyond both end velocities (two roots, or the double root within 1e-5 vm), between them, short of both.  As in the
// reference the candidate r carries the direction s already and is compared with s v0, s v1 and returned as s r.
RKH_HD bool svp_joint_peak(double p0, double p1, double v0, double v1, double vm, double T, double* peak) {
  *peak = v0;
  if (svp_same_point(p0, p1, v0, v1, vm)) return true;
  *peak = 0.0;
  if ((fabs(v0) > vm) || (fabs(v1) > vm)) return false;
  const double s = (p0 > p1) ? -1.0 : 1.0;
  const double sv0 = v0 * s, sv1 = v1 * s;
  {
    const double a = (v0 + v1) + T * s;
    const double c = vm * fabs(p1 - p0);
    const double q = 0.5 * (v0 * v0 + v1 * v1);
    const double aa = a * a, cq = 4.0 * (c + q);
    if (aa >= cq) {
      const double root = sqrt(aa - cq);
      double r = (0.5 * (a + root)) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r >= sv0) && (r >= sv1)) return *peak = s * r, true;
      r = (0.5 * (a - root)) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r >= sv0) && (r >= sv1)) return *peak = s * r, true;
    } else if (fabs(aa - cq) < 1e-5 * vm) {
      const double r = (0.5 * a) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r >= sv0) && (r >= sv1)) return *peak = s * r, true;
    }
  }
  {
    const double c = vm * (p1 - p0);
    if (v1 > v0) {  // two ramps up
      const double a = (v0 - v1) + T;
      const double q = 0.5 * (v0 * v0 - v1 * v1);
      if (fabs(a) > 1e-6 * vm) {
        const double vp = (c + q) / a;
        if (svp_peak_guard(vp, vp, v0, v1, vm, T) && (vp >= v0) && (vp <= v1)) return *peak = vp, true;
      }
    } else {  // two ramps down
      const double a = (v1 - v0) + T;
      const double q = 0.5 * (v1 * v1 - v0 * v0);
      if (fabs(a) > 1e-6 * vm) {
        const double vp = (c + q) / a;
        if (svp_peak_guard(vp, vp, v0, v1, vm, T) && (vp >= v1) && (vp <= v0)) return *peak = vp, true;
      }
    }
  }
  {
    const double a = (v0 + v1) - T * s;
    const double c = vm * fabs(p1 - p0);
    const double q = 0.5 * (v0 * v0 + v1 * v1);
    const double aa = a * a, qc = 4.0 * (q - c);
    if (aa > qc) {
      const double root = sqrt(aa - qc);
      double r = (0.5 * (a + root)) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r <= sv0) && (r <= sv1)) return *peak = s * r, true;
      r = (0.5 * (a - root)) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r <= sv0) && (r <= sv1)) return *peak = s * r, true;
    } else if (fabs(aa - qc) < 1e-5 * vm) {
      const double r = (0.5 * a) * s;
      if (svp_peak_guard(r, s * r, v0, v1, vm, T) && (r <= sv0) && (r <= sv1)) return *peak = s * r, true;
    }
  }
  return false;
}

// Position and velocity of one joint at time dt of the profile (peak vp, total time T): start, first ramp, cruise (the
// blend of the two ramp end positions, not an integration), second ramp, end.
RKH_HD void svp_joint_point(double p0, double p1, double v0, double v1, double vp, double vm, double dt, double T, double* p,
                            double* v) {
  double d1 = vp - v0, s1 = 1.0;
  if (vp < v0) s1 = -1.0, d1 = -d1;
  double d2 = v1 - vp, s2 = 1.0;
  if (v1 < vp) s2 = -1.0, d2 = -d2;
  const double cruise = T - (d2 + d1);
  if (dt <= 0.0) {
    *p = p0, *v = v0;
  } else if (dt < d1) {
    *p = p0 + ((v0 + (0.5 * dt) * s1) * dt) / vm;
    *v = v0 + dt * s1;
  } else if (dt < d1 + cruise) {
    const double w = (dt - d1) / cruise;
    const double ps = p0 + ((0.5 * (v0 + vp)) * d1) / vm;
    const double pe = p1 - ((0.5 * (vp + v1)) * d2) / vm;
    *p = w * pe + (1.0 - w) * ps;
    *v = vp;
  } else if (dt < (d1 + cruise) + d2) {
    const double m = ((d2 + d1) + cruise) - dt;
    *p = p1 - ((v1 - (0.5 * m) * s2) * m) / vm;
    *v = v1 - m * s2;
  } else {
    *p = p1, *v = v1;
  }
}

// Reach time d(a -> b) of two points: the largest of the joints' minimum times, if every joint has one, if every joint has
// a peak velocity that takes exactly that long, and if it is finite (coordinates that are not finite end here); else
// +inf.  peak (may be null): the peak velocities of the common-time solve, [n] at stride 1; zeros for +inf.
RKH_HD double svp_reach(const SvpDev& sp, const double* a, const double* b, double* peak) {
  const int n = sp.n;
  double T = 0.0;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    double t, vp;
    ok = svp_joint_min_time(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], sp.vm[i], &t, &vp) && ok;
    if (T < t) T = t;
  }
  ok = ok && (T < INFINITY);
  if (ok)
    for (int i = 0; i < n; ++i) {
      double vp;
      ok = svp_joint_peak(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], sp.vm[i], T, &vp) && ok;
      if (peak) peak[i] = vp;
    }
  if (!ok) {
    if (peak)
      for (int i = 0; i < n; ++i) peak[i] = 0.0;
    return INFINITY;
  }
  return T;
}

// The point at time dt of the profile of (a, b, peak, T), [2 n] to x; with scale, also in model units (p speed, v accel)
RKH_HD void svp_point(const SvpDev& sp, const double* a, const double* b, const double* peak, double T, double dt, double* x,
                      double* x_model) {
  for (int i = 0; i < sp.n; ++i) {
    double p, v;
    svp_joint_point(a[2 * i], b[2 * i], a[2 * i + 1], b[2 * i + 1], peak[i], sp.vm[i], dt, T, &p, &v);
    x[2 * i] = p, x[2 * i + 1] = v;
    if (x_model) x_model[2 * i] = p * sp.speed[i], x_model[2 * i + 1] = v * sp.accel[i];
  }
}

// The point, the point where each joint could stop and the point it could have started from are inside the position box,
// and the velocity inside +-vm (comparisons as hyperbox_out makes them).
RKH_HD bool svp_in_bounds(const SvpDev& sp, const double* x) {
  bool in = true;
  for (int i = 0; i < sp.n; ++i) {
    const double p = x[2 * i], v = x[2 * i + 1], vm = sp.vm[i], lo = sp.lower[i], hi = sp.upper[i];
    const double h = ((0.5 * v) * fabs(v)) / vm;
    in = in && !hyperbox_out(lo, hi, p) && !hyperbox_out(-vm, vm, v) && !hyperbox_out(lo, hi, p + h) &&
         !hyperbox_out(lo, hi, p - h);
  }
  return in;
}

// Tested points of an edge: the times d = min_interval, + min_interval, ... below dt, counted by the same repeated addition
// as the walk makes; at most cap (then *over is set: the caller refuses the edge instead of looping for ever).
RKH_HD uint32_t svp_count_points(double min_interval, double dt, uint32_t cap, bool* over) {
  uint32_t k = 0;
  double d = min_interval;
  *over = false;
  while (d < dt) {
    if (k == cap) {
      *over = true;
      break;
    }
    ++k;
    d += min_interval;
  }
  return k;
}

}  // namespace rkh
