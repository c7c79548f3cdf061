// propagate_depth.hip -- the depth forms of the record kernels (min_distance_depth_kernel, collision_depth_kernel: the
// two record kernels' bodies over pair_distance_depth / pair_record_depth of proximity_record_device.h, i.e. with the
// penetration depth and contact normal of epa_device.h for vertex-set pairs) and the pair-by-pair gjk_pair_depth_kernel of
// the diagnostic entry: propagate.hip compiled with RKH_DEPTH_RECORDS, under which it instantiates these kernels with
// their three launchers and none of its other kernels or launchers.  A module of their own: the polytope arrays give
// them a private segment, and a kernel added to propagate.hip's module has moved the registers of the ones it holds.
#define RKH_DEPTH_RECORDS 1
#include "propagate.hip"
