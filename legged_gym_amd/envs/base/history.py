"""Layout of the actor's observation row with a history: `[obs | frame_1 | ... | frame_H]`.

The reference has no observation history, so there are no reference semantics to follow: the
layout is this project's own.  `obs` is the `num_obs`-wide row the env returns
without a history (noisy, clipped); `frame_k` is the first `frame_width` entries of the `obs` part of
the row the same env returned `k` steps ago, as the actor saw them - or zeros where that row lies
before the current episode's first one.

Pure Python (no torch, no library): this module is the one place that knows the row's arithmetic.
"""

from legged_gym_amd.sim.abi import MAX_PRIV_OBS as MAX_WIDTH   # the rollout MLP's input limit (rl/actor_critic.py)


class Layout:
    """frames: H >= 1; frame_width: W; width: num_obs + H * W floats per row."""

    def __init__(self, num_obs, frames, frame_width):
        self.num_obs, self.frames, self.frame_width = num_obs, frames, frame_width
        self.width = num_obs + frames * frame_width
        self.obs = slice(0, num_obs)
        self.tail = slice(num_obs, self.width)

    def frame(self, k):
        """Columns of frame k (1 = the previous step's row ... frames = the oldest)."""
        if not 1 <= k <= self.frames:
            raise ValueError(f"frame {k} of a history of {self.frames} frames")
        start = self.num_obs + (k - 1) * self.frame_width
        return slice(start, start + self.frame_width)

    def source(self, k):
        """Columns of the previous row that frame k is copied from: its obs part for frame 1, its
        frame k - 1 otherwise."""
        return slice(0, self.frame_width) if k == 1 else self.frame(k - 1)


def layout(frames, frame_width, num_obs):
    """The row layout of `frames` frames of `frame_width` behind `num_obs` observations, or None for
    frames == 0 (no history: the row is the observations alone).  ValueError for frames < 0, a frame
    width outside [1, num_obs], or a row wider than MAX_WIDTH."""
    frames = int(frames)
    if frames < 0:
        raise ValueError(f"history.frames = {frames}; it must be >= 0")
    if frames == 0:
        return None
    frame_width = int(frame_width)
    if not 1 <= frame_width <= num_obs:
        raise ValueError(f"history.frame_width = {frame_width}; a frame is the leading entries of the observation "
                         f"row, so it must lie in [1, num_observations = {num_obs}]")
    width = num_obs + frames * frame_width
    if width > MAX_WIDTH:
        raise ValueError(f"observation row of {width} entries (num_observations {num_obs} + {frames} frames of "
                         f"{frame_width}); the limit is {MAX_WIDTH} (the rollout MLP's input width)")
    return Layout(num_obs, frames, frame_width)
