"""The command curriculum restated in numpy float64 (tests only), written from the rule itself
(legged_gym/envs/base/legged_robot.py:165-167, 189-190, 465-474 and _resample_commands :354-368):

  in reset_idx(env_ids), before the commands of env_ids are resampled:
    if commands.curriculum and len(env_ids) > 0 and common_step_counter % max_episode_length == 0:
      if mean(episode_sums["tracking_lin_vel"][env_ids]) / max_episode_length > 0.8 * scale:
        lo = clip(lo - 0.5, -max_curriculum, 0);  hi = clip(hi + 0.5, 0, max_curriculum)
  then env_ids draw x, y from the (new) ranges; commands with |xy| <= 0.2 m/s are zeroed.

The draws are inputs (uniform numbers in [0, 1), one per command slot), so the device's Philox
stream or injected draws can be replayed.  Nothing here reads the code under test.
"""
import numpy as np

STEP = 0.5
FRACTION = 0.8
GATE = 0.2            # m/s: the small-command gate over x and y
DRAW_CMD = 0          # LGX_DRAW_CMD: the periodic resample's slots (x, y, yaw | heading)
DRAW_RESET_CMD = 25   # LGX_DRAW_RESET_CMD: the reset's slots
DRAW_NOISE = 32       # LGX_DRAW_NOISE: a draw row is DRAW_NOISE + num_obs wide


def is_curriculum_step(common_step_counter, max_episode_length):
    return common_step_counter % float(max_episode_length) == 0


def widen(lo, hi, max_curriculum):
    """One widening of [lo, hi] (np.clip's own semantics, also for a start outside the interval)."""
    return (float(np.clip(lo - STEP, -max_curriculum, 0.0)), float(np.clip(hi + STEP, 0.0, max_curriculum)))


def lhs(sums_of_reset_envs, max_episode_length):
    """The left side in float64 (the device's is float32: compare within the summation bound)."""
    s = np.asarray(sums_of_reset_envs, dtype=np.float64)
    return float(s.mean() / float(max_episode_length))


def decide(lo, hi, count, sums_of_reset_envs, common_step_counter, max_episode_length, scale, max_curriculum,
           enabled=True):
    """-> (lo, hi, count, lhs or None).  scale: reward_scales["tracking_lin_vel"], dt included (float64);
    the comparison is float32 against float32(0.8 * scale), as torch makes it.  count: how often the
    range moved."""
    s = np.asarray(sums_of_reset_envs, dtype=np.float64)
    if not enabled or s.size == 0 or not is_curriculum_step(common_step_counter, max_episode_length):
        return lo, hi, count, None
    left = lhs(s, max_episode_length)
    if np.float32(left) > np.float32(FRACTION * float(scale)):
        nlo, nhi = widen(lo, hi, max_curriculum)
        if (nlo, nhi) != (lo, hi):
            lo, hi, count = nlo, nhi, count + 1
    return lo, hi, count, left


def draw_xy(u_x, u_y, range_x, range_y):
    """The x, y command of one env from its two uniform draws: (hi - lo) * u + lo, then the gate."""
    u_x, u_y = np.asarray(u_x, dtype=np.float64), np.asarray(u_y, dtype=np.float64)
    cx = (range_x[1] - range_x[0]) * u_x + range_x[0]
    cy = (range_y[1] - range_y[0]) * u_y + range_y[0]
    keep = (np.sqrt(cx * cx + cy * cy) > GATE).astype(np.float64)
    return cx * keep, cy * keep
