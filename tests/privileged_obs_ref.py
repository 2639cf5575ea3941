"""Plain-torch statement of the privileged observation row, over the env's public tensors as they
are after a step returns.  The reference (legged_gym) never fills its privileged buffer, so this is
NOT a restatement of reference semantics: it states this project's own layout (DESIGN.md,
envs/base/privileged.py) independently of the kernel that writes it.

  row = [clean | tail]
  clean: compute_observations (legged_robot.py:217-228) without the noise of :230-231, in its op
         order, then the clip of :103-104
  tail:  cfg.privileged.terms in order, each clipped the same way

Every entry is one float32 subtract and one float32 multiply (no fused multiply-add can form), so
the kernel's row is expected to be bitwise this one.
"""
import torch


def clean_obs(env):
    """The observation row before noise and clip (legged_robot.py:217-228)."""
    s = env.obs_scales
    obs = torch.cat((env.base_lin_vel * s.lin_vel,
                     env.base_ang_vel * s.ang_vel,
                     env.projected_gravity,
                     env.commands[:, :3] * env.commands_scale,
                     (env.dof_pos - env.default_dof_pos) * s.dof_pos,
                     env.dof_vel * s.dof_vel,
                     env.actions), dim=-1)
    if env.cfg.terrain.measure_heights:
        heights = torch.clip(env.root_states[:, 2].unsqueeze(1) - 0.5 - env.measured_heights, -1, 1.) \
            * s.height_measurements
        obs = torch.cat((obs, heights), dim=-1)
    return obs


def tail_term(env, name):
    p = env.cfg.privileged
    feet = env.feet_indices
    if name == "friction":
        return env.friction_coeffs.unsqueeze(1)
    if name == "base_mass":
        return env.body_mass_scale[:, :1]
    if name == "mass_scale":
        return env.body_mass_scale
    if name == "feet_contact":
        return (env.contact_forces[:, feet, 2] > 1.).float()
    if name == "feet_forces":
        return (env.contact_forces[:, feet, :] * p.contact_force_scale).flatten(1)
    if name == "torques":
        return env.torques * p.torque_scale
    raise KeyError(name)


def privileged_obs_ref(env):
    """[N, num_obs + tail width]: what env.privileged_obs_buf must hold after the step that left
    the public tensors in their current state."""
    clip = env.cfg.normalization.clip_observations
    row = torch.cat([clean_obs(env)] + [tail_term(env, t) for t in env.cfg.privileged.terms], dim=-1)
    return torch.clip(row, -clip, clip)
