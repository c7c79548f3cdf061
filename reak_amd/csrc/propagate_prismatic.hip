// propagate_prismatic.hip -- the forms of the one-wave-per-edge steer kernel, the f-eval kernel, the distance query and
// the 3D edge walk for scenes with prismatic joints (SceneDev::has_prismatic): propagate.hip compiled a second time with
// RKH_PRISMATIC_FORMS, its kernels and launchers in rkh::prismatic.  A translation unit of its own keeps the revolute
// kernels of propagate.hip exactly as they were (their code does not depend on what else is instantiated next to them).
#define RKH_PRISMATIC_FORMS
#include "propagate.hip"
