// propagate_planar_qs_prismatic.hip -- the position-level forms (quasi-static edge walk, distance query) for planar chains
// with prismatic_joint_2D groups (SceneDev::planar && has_prismatic): propagate.hip compiled with RKH_PLANAR_PRISMATIC_QS,
// under which it instantiates rkh::planar_prismatic::edge_check_kernel / min_distance_kernel with their two launchers and
// none of its other kernels or launchers.
#define RKH_PLANAR_PRISMATIC_QS 1
#include "propagate.hip"
