// propagate_pair_prismatic.hip -- the forms of the two-lanes-per-edge steer kernels (whole edges, one RK4 step per launch)
// and of the proximity-count probe for chains with prismatic joints (SceneDev::has_prismatic): propagate_pair.hip compiled
// a second time with RKH_PRISMATIC_FORMS, its kernels and launchers in rkh::prismatic.  A translation unit of its own
// keeps the revolute kernels of propagate_pair.hip exactly as they were.
#define RKH_PRISMATIC_FORMS
#include "propagate_pair.hip"
