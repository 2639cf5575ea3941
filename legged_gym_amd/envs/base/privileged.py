"""Layout of the privileged (critic-only) observation row: `[clean | tail]`.

The reference declares the buffer (`cfg.env.num_privileged_obs`, base_task.py:75-78), clips it
(legged_robot.py:103-106) and returns it from `step` / `reset`, but its `compute_observations`
never fills it, so there are no reference semantics to follow: the layout is this project's own
(DESIGN.md).  `clean` is the `num_obs`-wide observation row before noise; `tail` is the terms of
`cfg.privileged.terms` in that order, each clipped to +-clip_observations like the rest of the row.

Pure Python (no torch, no library): this module is the one place that knows the terms' names and widths.
"""

from legged_gym_amd.sim.abi import MAX_PRIV_OBS as MAX_WIDTH   # the rollout MLP's input limit (rl/actor_critic.py)
from legged_gym_amd.sim.abi import NUM_DOF, NUM_DYN, PRIV_MAX_TERMS as MAX_TERMS, PRIV_TERM_IDS

# name -> width given the number of feet (values: include/lgx.h, enum lgx_priv_term)
WIDTHS = {
    "friction": lambda num_feet: 1,                 # friction_coeffs[e]
    "base_mass": lambda num_feet: 1,                # body_mass_scale[e, 0]
    "mass_scale": lambda num_feet: NUM_DYN,         # body_mass_scale[e, :]
    "feet_contact": lambda num_feet: num_feet,      # contact_forces[e, feet, 2] > 1
    "feet_forces": lambda num_feet: 3 * num_feet,   # contact_forces[e, feet, :] * contact_force_scale
    "torques": lambda num_feet: NUM_DOF,            # torques[e, :] * torque_scale
}
TERMS = {name: (PRIV_TERM_IDS[name], width) for name, width in WIDTHS.items()}


class Layout:
    """terms: [(name, term id, slice into the row)], in row order; width: floats per row."""

    def __init__(self, num_obs, terms, width):
        self.num_obs, self.terms, self.width = num_obs, terms, width
        self.clean = slice(0, num_obs)

    @property
    def tail_width(self):
        return self.width - self.num_obs

    def slices(self):
        return {name: sl for name, _, sl in self.terms}


def layout(terms, num_obs, num_feet, num_privileged_obs=None):
    """The row layout of `terms` behind `num_obs` clean entries.  ValueError for an unknown or
    repeated term, a row wider than MAX_WIDTH, or (when given) a `num_privileged_obs` that is not
    `num_obs` + the tail's width."""
    terms = tuple(terms)
    out, off = [], num_obs
    for name in terms:
        if name not in TERMS:
            raise ValueError(f"unknown privileged observation term {name!r}; known terms: {', '.join(TERMS)}")
        if name in [n for n, _, _ in out]:
            raise ValueError(f"privileged observation term {name!r} is listed twice")
        tid, width = TERMS[name]
        w = width(num_feet)
        out.append((name, tid, slice(off, off + w)))
        off += w
    if len(out) > MAX_TERMS:
        raise ValueError(f"{len(out)} privileged observation terms; the limit is {MAX_TERMS}")
    if num_privileged_obs is not None and num_privileged_obs != off:
        raise ValueError(f"env.num_privileged_obs = {num_privileged_obs}, but num_observations ({num_obs}) + the "
                         f"privileged terms {terms} ({off - num_obs}) = {off}")
    if off > MAX_WIDTH:
        raise ValueError(f"privileged observation row of {off} entries; the limit is {MAX_WIDTH} "
                         "(the rollout MLP's input width)")
    return Layout(num_obs, out, off)
