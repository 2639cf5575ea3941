// The physics kernel with per-env actuator tables bound (lgx_bind_actuator_rand): the
// lgx_physics_kernel<PP, lgx_act_rand_args> instantiations of lgx_physics.hip and their launcher, as a
// translation unit of their own (why: the note above `#ifdef LGX_PHYSICS_RAND` in that file).
#define LGX_PHYSICS_RAND 1
#include "lgx_physics.hip"
