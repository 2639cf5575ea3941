// The post-physics kernels with an observation history bound (lgx_bind_obs_history): the history
// instantiations of lgx_envlogic.hip's post_physics_body and the launcher's choice among them, as
// a translation unit of their own (why: the note above `#ifndef LGX_ENVLOGIC_HIST` in that file).
#define LGX_ENVLOGIC_HIST 1
#include "lgx_envlogic.hip"
