// Stand-in for <hip/hip_runtime.h> on a host compiler: just enough for g++ to read the device headers that use no
// device builtin beyond these (device_math.h, gjk_device.h, proximity_device.h, proximity_record_device.h), so that
// their closed forms run on the CPU under test (prox_record_host.cpp).  Only ever found through -I tests/cpp/hip_host.
#pragma once
#include <math.h>
#include <stdint.h>

#define __device__
#define __host__
#define __forceinline__ inline

inline double __shfl(double v, int, int) { return v; }  // device_math.h's bcast: one "lane" on the host
