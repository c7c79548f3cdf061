// propagate_planar_prismatic.hip -- the forms of the planar steer and f-eval kernels for chains with prismatic_joint_2D
// groups (SceneDev::planar && has_prismatic): propagate_planar.hip compiled a second time with RKH_PLANAR_PRISMATIC_FORMS,
// which puts its kernels and launchers into rkh::planar_prismatic and turns the prismatic branches of its joint loops on.
#define RKH_PLANAR_PRISMATIC_FORMS 1
#include "propagate_planar.hip"
