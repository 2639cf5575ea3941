"""Command curriculum (cfg.commands.curriculum; legged_robot.py:165-167, 189-190, 465-474): the host's
share of it.  The decision and the resample run on the device (lgx_bind_command_curriculum,
csrc/lgx_cmd_curriculum.hip); the host knows, from the step counter alone, on which
steps they run, and prepares the two numbers of the rule.
"""
import math

import numpy as np

RANGE_NAMES = ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "heading")   # lgx_env_params.cmd_ranges rows
STEP = 0.5               # the reference widens each bound by 0.5 m/s
FRACTION = 0.8           # ... once tracking_lin_vel reaches 80 % of its maximum
COMMAND_COLUMNS = slice(9, 12)   # the commands' entries of an observation row


def is_curriculum_step(common_step_counter, max_episode_length):
    """`common_step_counter % max_episode_length == 0` (legged_robot.py:165) with the integer-valued
    float length of the reference; counter 0 is such a step.  The library applies the same test
    (lgx_is_curriculum_step)."""
    length = float(max_episode_length)
    if not length > 0:
        return False
    return int(common_step_counter) % length == 0


def threshold(tracking_scale):
    """The right-hand side of the comparison: the reference's float64 product 0.8 * scale (the scale
    already holds dt), which torch compares as float32."""
    return np.float32(FRACTION * float(tracking_scale))


def validate(commands_cfg, reward_scales, noise_scale_vec):
    """(max_curriculum, threshold) for an env with commands.curriculum set; ValueError for a config
    the rule cannot run on.  reward_scales: the env's dict after _prepare_reward_function (zero
    scales dropped, the rest times dt)."""
    scale = reward_scales.get("tracking_lin_vel")
    if scale is None or not scale > 0:
        raise ValueError("commands.curriculum reads the tracking_lin_vel episode sum: rewards.scales.tracking_lin_vel "
                         f"must be > 0 (got {0.0 if scale is None else scale}; the reference raises KeyError)")
    mx = float(commands_cfg.max_curriculum)
    if not math.isfinite(mx) or mx < 0:
        raise ValueError(f"commands.max_curriculum = {commands_cfg.max_curriculum}: must be finite and >= 0")
    nz = np.asarray(noise_scale_vec, dtype=np.float64)[COMMAND_COLUMNS]
    if np.any(nz != 0):
        raise ValueError(f"commands.curriculum: the command columns of noise_scale_vec must be zero (got {nz.tolist()}); "
                         "the reference zeroes them, and the resample rewrites those observation entries")
    return mx, threshold(scale)
