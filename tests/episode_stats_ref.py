"""rsl_rl OnPolicyRunner.learn's episode bookkeeping (the torch / deque block of the runner's
collection loop), restated as the reference of the EpisodeStats tests, and their shared inputs."""
from collections import deque

import torch


class DequeStats:
    def __init__(self, num_envs, device, capacity=100):
        self.rewbuffer = deque(maxlen=capacity)
        self.lenbuffer = deque(maxlen=capacity)
        self.cur_reward_sum = torch.zeros(num_envs, dtype=torch.float, device=device)
        self.cur_episode_length = torch.zeros(num_envs, dtype=torch.float, device=device)

    def step(self, rewards, dones):
        self.cur_reward_sum += rewards
        self.cur_episode_length += 1
        new_ids = (dones > 0).nonzero(as_tuple=False)
        self.rewbuffer.extend(self.cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
        self.lenbuffer.extend(self.cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0

    def lists(self):
        return list(self.rewbuffer), list(self.lenbuffer)


def random_sequence(num_envs=1025, steps=40, p=0.03, all_done_step=17, seed=0):
    """[(rewards float32 [N], dones bool [N])] on the CPU: randn rewards, Bernoulli(p) dones, one
    step with every env done."""
    g = torch.Generator().manual_seed(seed)
    seq = []
    for t in range(steps):
        rew = torch.randn(num_envs, generator=g)
        dones = torch.rand(num_envs, generator=g) < p
        if t == all_done_step:
            dones[:] = True
        seq.append((rew, dones))
    return seq
