"""Reference model of the observation history (include/lgx.h): plain torch that
replays the rule from what the env returns - the `obs` part of each row, `reset_buf` of that step
and the explicit `reset_idx` calls between steps.

    a        = 0 where reset_buf (this step) else age
    frame_k  = the previous row's frame k - 1 (its leading W obs entries for k = 1) if k <= a else 0
    age      = min(a + 1, H)

`reset_idx(ids)` sets age = 0 and touches no row.  Ages and the previous row start at zero.
"""
import torch


class ObsHistoryRef:
    def __init__(self, num_envs, num_obs, frames, frame_width, device="cpu"):
        self.num_obs, self.frames, self.frame_width = num_obs, frames, frame_width
        self.width = num_obs + frames * frame_width
        self.age = torch.zeros(num_envs, dtype=torch.int64, device=device)
        self.prev = torch.zeros(num_envs, self.width, dtype=torch.float32, device=device)
        self.last_a = self.age.clone()      # the a of the last step, for the tests' coverage checks

    def reset_idx(self, ids):
        self.age[torch.as_tensor(ids, dtype=torch.int64, device=self.age.device)] = 0

    def step(self, obs, reset_buf):
        """obs [N, num_obs]: the obs part of the row returned this step; -> the whole expected row."""
        W, no = self.frame_width, self.num_obs
        a = torch.where(reset_buf.bool(), torch.zeros_like(self.age), self.age)
        row = torch.zeros_like(self.prev)
        row[:, :no] = obs
        for k in range(1, self.frames + 1):
            src = self.prev[:, :W] if k == 1 else self.prev[:, no + (k - 2) * W:no + (k - 1) * W]
            row[:, no + (k - 1) * W:no + k * W] = torch.where((k <= a)[:, None], src, torch.zeros_like(src))
        self.age = (a + 1).clamp(max=self.frames)
        self.prev, self.last_a = row, a
        return row
