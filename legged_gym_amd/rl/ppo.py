"""PPO with the rsl_rl v1.0.x algorithm and hyper-parameter contract
(legged_robot_config.py:226-239; upstream rsl_rl `PPO`), data-parallel over ranks.

Data parallelism (new; the reference is single-GPU): every rank owns its envs and a full
ActorCritic replica.  Per minibatch the flat fp32 gradient is all-reduced (RCCL over xGMI when
the process group backend is "nccl") and averaged before clip_grad_norm, advantage
normalisation uses global statistics, and the KL used by the adaptive learning rate is the
global mean, so every rank applies the identical Adam step and N ranks x B envs reproduce
1 rank x N*B envs up to reduction order.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.optim as optim

from .actor_critic import ActorCritic
from .fused_ppo import FusedPPOUpdate
from .fused_rollout import FusedRollout
from .storage import RolloutStorage


def _dist():
    """torch.distributed when the job runs data-parallel (world > 1).  LGX_DIST_REHEARSAL=1 takes the
    data-parallel path at world 1 too (every collective over a one-rank RCCL communicator): the
    single-GPU rehearsal of the multi-GPU code path (bench.py, tests/test_gpu_ddp.py)."""
    import os
    import torch.distributed as dist
    least = 1 if os.environ.get("LGX_DIST_REHEARSAL") == "1" else 2
    return dist if dist.is_available() and dist.is_initialized() and dist.get_world_size() >= least else None


def _symmetry_cfg(cfg):
    """algorithm.symmetry (None, a dict or a config object) -> (whether data augmentation is on, the
    mirror loss's coefficient or None with the mirror loss off).  ValueError for a key this
    implementation does not know, and for use_mirror_loss = True without a mirror_loss_coeff that
    is a finite number > 0 (rsl_rl 2.x indexes symmetry_cfg["mirror_loss_coeff"] and fails too).
    With use_mirror_loss off the coefficient is ignored (rsl_rl 2.x logs a detached symmetry loss
    then; nothing is computed here)."""
    if cfg is None:
        return False, None
    d = dict(cfg) if isinstance(cfg, dict) else {k: getattr(cfg, k) for k in dir(cfg) if not k.startswith("_")}
    unknown = sorted(set(d) - {"use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff"})
    if unknown:
        raise ValueError(f"symmetry: unsupported key(s) {unknown} (use_data_augmentation, use_mirror_loss and "
                         "mirror_loss_coeff are implemented)")
    coeff = None
    if d.get("use_mirror_loss", False):
        coeff = d.get("mirror_loss_coeff")
        if isinstance(coeff, bool) or not isinstance(coeff, (int, float)) or not (0.0 < coeff < float("inf")):
            raise ValueError(f"symmetry: use_mirror_loss = True needs mirror_loss_coeff, a finite number > 0 "
                             f"(got {coeff!r})")
        coeff = float(coeff)
    return bool(d.get("use_data_augmentation", False)), coeff


class PPO:
    actor_critic: ActorCritic

    def __init__(self, actor_critic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu", use_fused_update=True,
                 symmetry=None):
        """symmetry: None, or the `algorithm.symmetry` config as a dict (class_to_dict) or an object with
        attributes.  use_data_augmentation = True trains every minibatch on its rollout rows and their
        left-right mirror images (rsl_rl 2.x symmetry_cfg.use_data_augmentation).
        use_mirror_loss = True with mirror_loss_coeff = c adds c x the actor's equivariance defect on
        every minibatch, mean((mu(mirror(o)) - mirror(mu(o)).detach())^2), to the loss (rsl_rl 2.x
        symmetry_cfg.use_mirror_loss); without augmentation the PPO terms then run
        over the rollout rows alone and the mirror rows carry only that term.  With either flag on
        the caller hands the env's tables to init_symmetry() before init_storage().  Off, None and
        absent all mean nothing changes."""
        self.device = device
        # symmetry: the storage holds the rows' mirror images (either flag); symmetry_augment: the PPO
        # terms run over them too; mirror_loss_coeff: None, or the mirror loss's coefficient
        self.symmetry_augment, self.mirror_loss_coeff = _symmetry_cfg(symmetry)
        self.symmetry = self.symmetry_augment or self.mirror_loss_coeff is not None
        self.symmetry_tables = None
        self.symmetry_loss = None   # the last update's mean symmetry loss (mirror loss on)
        if self.symmetry and actor_critic.is_recurrent:
            raise ValueError("symmetry.use_data_augmentation / use_mirror_loss: recurrent policies are not supported "
                             "(a mirrored trajectory needs its own memory states)")
        self.desired_kl = desired_kl
        self.schedule = schedule
        self.learning_rate = learning_rate
        self.actor_critic = actor_critic.to(self.device)
        self.storage = None
        fused = str(device).startswith("cuda")
        self.optimizer = optim.Adam(self.actor_critic.parameters(), lr=learning_rate, fused=fused or None)
        self.transition = RolloutStorage.Transition()
        self.clip_param = clip_param
        self.num_learning_epochs = num_learning_epochs
        self.num_mini_batches = num_mini_batches
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.gamma = gamma
        self.lam = lam
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.dist = _dist()
        self._fused = self._rollout = self._deferred = None
        # process_env_step leaves its storage-row launch to the next act (one launch per step);
        # set by OnPolicyRunner, whose loop always calls act between env.step calls
        self.defer_store = False
        if fused and use_fused_update and FusedPPOUpdate.supported(self.actor_critic):
            self._fused = FusedPPOUpdate(self)       # parameters become views of its flat buffer
            self.optimizer = self._fused.optimizer
            if FusedRollout.supported(self.actor_critic):
                self._rollout = FusedRollout(self, self._fused.lib)
        if self.dist is not None:
            self._broadcast_params()

    # ---------------------------------------------------------------- setup / modes
    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        if self.symmetry and self.symmetry_tables is None:
            raise ValueError("symmetry.use_data_augmentation / use_mirror_loss is on: call "
                             "init_symmetry(env.symmetry_tables()) before init_storage()")
        if self.symmetry:
            for key, shape in (("obs", actor_obs_shape), ("critic_obs", critic_obs_shape), ("actions", action_shape)):
                t = self.symmetry_tables[key]
                if (t is None) != (shape[0] is None) or (t is not None and t[0].numel() != shape[0]):
                    raise ValueError(f"symmetry: the {key} table is {None if t is None else t[0].numel()} wide, the "
                                     f"storage's rows {shape[0]}")
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape,
                                      action_shape, self.device, symmetry=self.symmetry_tables)

    def init_symmetry(self, tables):
        """The env's mirror tables (LeggedRobot.symmetry_tables(): {"obs", "critic_obs" or None,
        "actions"} -> (perm int32, sign float32)), moved to this algorithm's device and checked once
        (every perm entry in range, every sign +-1); ValueError with symmetry off."""
        if not self.symmetry:
            raise ValueError("init_symmetry: symmetry.use_data_augmentation and use_mirror_loss are off")
        tables = {k: None if v is None else (v[0].to(self.device, torch.int32).contiguous(),
                                             v[1].to(self.device, torch.float32).contiguous())
                  for k, v in tables.items()}
        for key, t in tables.items():
            if t is None:
                continue
            perm, sign = t[0].cpu(), t[1].cpu()
            if self._fused is not None:   # the library's own check of what its launch will trust
                self._fused.check(self._fused.lib.lgx_ppo_symmetry_check_table(
                    C.c_void_p(perm.data_ptr()), C.c_void_p(sign.data_ptr()), perm.numel()), "symmetry_check_table")
            elif (perm.numel() != sign.numel() or not ((perm >= 0) & (perm < perm.numel())).all()
                  or not (sign.abs() == 1).all()):
                raise ValueError(f"symmetry: the {key} table is not a signed permutation")
        self.symmetry_tables = tables

    def test_mode(self):
        self.actor_critic.test()

    def train_mode(self):
        self.actor_critic.train()

    def _broadcast_params(self):
        with torch.no_grad():
            for p in self.actor_critic.parameters():
                self.dist.broadcast(p.data, src=0)

    # ---------------------------------------------------------------- rollout
    def act(self, obs, critic_obs):
        if self._rollout is not None:   # actions, values and the storage rows from the kernels
            actions = self._rollout.act(obs, critic_obs)
            if actions is not None:
                return actions
        t = self.transition
        self.flush_store()   # (a deferred store reads the env's buffers before the next env.step)
        if self.actor_critic.is_recurrent:   # the memories' state before this step (rsl_rl PPO.act)
            t.hidden_states = self.actor_critic.get_hidden_states()
        if hasattr(self.actor_critic, "act_and_evaluate"):
            actions, values = self.actor_critic.act_and_evaluate(obs, critic_obs)
            t.actions, t.values = actions.detach(), values.detach()
        else:
            t.actions = self.actor_critic.act(obs).detach()
            t.values = self.actor_critic.evaluate(critic_obs).detach()
        t.actions_log_prob = self.actor_critic.get_actions_log_prob(t.actions).detach()
        t.action_mean = self.actor_critic.action_mean.detach()
        t.action_sigma = self.actor_critic.action_std.detach()
        t.observations = obs
        t.critic_observations = critic_obs
        return t.actions

    def process_env_step(self, rewards, dones, infos):
        t = self.transition
        if t.in_storage:     # the other rows already written by FusedRollout.act
            self._rollout.store(rewards, dones, infos)
            self.storage.step += 1
        else:
            t.rewards = rewards.clone()
            t.dones = dones
            if "time_outs" in infos:  # bootstrap on time-outs
                t.rewards += self.gamma * torch.squeeze(t.values * infos["time_outs"].unsqueeze(1).to(self.device), 1)
            self.storage.add_transitions(t)
        t.clear()
        self.actor_critic.reset(dones)

    @property
    def last_act_fused(self):   # the last kernel-driven act was the one fused launch (False before it, and on CPU)
        return self._rollout is not None and self._rollout.last_fused

    def flush_store(self):
        """Launch a deferred process_env_step store (defer_store) on its own."""
        if self._rollout is not None:
            self._rollout.flush()

    def drop_store(self):
        """Forget a deferred store without launching it (cleanup after an error)."""
        if self._rollout is not None:
            self._rollout.drop()

    def _gather_moments(self, parts):
        """Every rank's flat float64 (count, mean, M2) advantage summaries, concatenated in rank order
        (all_gather: identical on every rank, so every rank normalises with the same statistics)."""
        parts = parts.contiguous()
        if self.dist is None:
            return parts
        out = [torch.empty_like(parts) for _ in range(self.dist.get_world_size())]
        self.dist.all_gather(out, parts)
        return torch.cat(out)

    def compute_returns(self, last_critic_obs):
        self.flush_store()
        last_values = self.actor_critic.evaluate(last_critic_obs).detach()
        self.storage.compute_returns(last_values, self.gamma, self.lam,
                                     reduce_stats=self._gather_moments if self.dist is not None else None)

    # ---------------------------------------------------------------- update
    def _allreduce_grads(self):
        params = [p for p in self.actor_critic.parameters() if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        self.dist.all_reduce(flat)
        flat /= self.dist.get_world_size()
        off = 0
        for p in params:
            n = p.grad.numel()
            p.grad.copy_(flat[off:off + n].view_as(p.grad))
            off += n

    def minibatch_loss(self, batch):
        """The unfused path's forward and loss of one minibatch of the storage's generators -> (loss,
        value loss, surrogate loss, symmetry loss or None, (mu, sigma, old mu, old sigma) of the rows
        the PPO terms - and the adaptive schedule's KL - run over)."""
        obs_b, cobs_b, act_b, target_v_b, adv_b, ret_b, old_logp_b, old_mu_b, old_sigma_b, hid_b, masks_b = batch
        self.actor_critic.act(obs_b, masks=masks_b, hidden_states=hid_b[0])
        logp_b = self.actor_critic.get_actions_log_prob(act_b)
        value_b = self.actor_critic.evaluate(cobs_b, masks=masks_b, hidden_states=hid_b[1])
        mu_b = self.actor_critic.action_mean
        sigma_b = self.actor_critic.action_std
        entropy_b = self.actor_critic.entropy
        symmetry_loss = None
        if self.mirror_loss_coeff is not None:
            # the minibatch is M rollout rows, then their M mirror images: the mirror rows' mean against
            # the mirrored mean of the rollout rows (the target: no gradient through it)
            M = mu_b.shape[0] // 2
            act_perm, act_sign = self.symmetry_tables["actions"]
            target = mu_b[:M].detach()[:, act_perm.long()] * act_sign
            symmetry_loss = nn.functional.mse_loss(mu_b[M:], target)
            if not self.symmetry_augment:   # the PPO terms over the rollout rows alone
                (logp_b, value_b, mu_b, sigma_b, entropy_b, target_v_b, adv_b, ret_b, old_logp_b, old_mu_b,
                 old_sigma_b) = (x[:M] for x in (logp_b, value_b, mu_b, sigma_b, entropy_b, target_v_b, adv_b, ret_b,
                                                 old_logp_b, old_mu_b, old_sigma_b))
        ratio = torch.exp(logp_b - torch.squeeze(old_logp_b))
        adv = torch.squeeze(adv_b)
        surrogate = -adv * ratio
        surrogate_clipped = -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
        surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
        if self.use_clipped_value_loss:
            value_clipped = target_v_b + (value_b - target_v_b).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((value_b - ret_b).pow(2), (value_clipped - ret_b).pow(2)).mean()
        else:
            value_loss = (ret_b - value_b).pow(2).mean()
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * entropy_b.mean()
        if symmetry_loss is not None:
            loss = loss + self.mirror_loss_coeff * symmetry_loss
        return loss, value_loss, surrogate_loss, symmetry_loss, (mu_b, sigma_b, old_mu_b, old_sigma_b)

    def update(self, defer=False):
        """rsl_rl PPO.update -> (mean value loss, mean surrogate loss).  defer=True (fused path only)
        issues the update and returns None; resolve() returns the losses later (FusedPPOUpdate)."""
        self.flush_store()
        if self._fused is not None:
            out = self._fused.update(defer=defer)
            self.storage.clear()
            if hasattr(self.actor_critic, "invalidate_fused"):
                self.actor_critic.invalidate_fused()
            return out
        mean_value_loss = 0.0
        mean_surrogate_loss = 0.0
        mean_symmetry_loss = 0.0
        if self.actor_critic.is_recurrent:
            gen = self.storage.reccurent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        else:
            gen = self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        for batch in gen:
            loss, value_loss, surrogate_loss, symmetry_loss, (mu_b, sigma_b, old_mu_b, old_sigma_b) = \
                self.minibatch_loss(batch)
            # (the schedule only sets the step's learning rate: after the loss or before it, as upstream)
            if self.desired_kl is not None and self.schedule == "adaptive":
                with torch.inference_mode():
                    kl = torch.sum(torch.log(sigma_b / old_sigma_b + 1.e-5) +
                                   (torch.square(old_sigma_b) + torch.square(old_mu_b - mu_b)) /
                                   (2.0 * torch.square(sigma_b)) - 0.5, axis=-1)
                    kl_mean = torch.mean(kl)
                    if self.dist is not None:
                        self.dist.all_reduce(kl_mean)
                        kl_mean /= self.dist.get_world_size()
                    kl_mean = kl_mean.item()
                    if kl_mean > self.desired_kl * 2.0:
                        self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                    elif self.desired_kl / 2.0 > kl_mean > 0.0:
                        self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                    for g in self.optimizer.param_groups:
                        g["lr"] = self.learning_rate
            if symmetry_loss is not None:
                mean_symmetry_loss += symmetry_loss.detach()
            self.optimizer.zero_grad()
            loss.backward()
            if self.dist is not None:
                self._allreduce_grads()
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.optimizer.step()
            mean_value_loss += value_loss.detach()
            mean_surrogate_loss += surrogate_loss.detach()
        if hasattr(self.actor_critic, "invalidate_fused"):
            self.actor_critic.invalidate_fused()
        n = self.num_learning_epochs * self.num_mini_batches
        mean_value_loss = (mean_value_loss / n).item()
        mean_surrogate_loss = (mean_surrogate_loss / n).item()
        if self.mirror_loss_coeff is not None:
            self.symmetry_loss = (mean_symmetry_loss / n).item()
        self.storage.clear()
        if defer:
            self._deferred = (mean_value_loss, mean_surrogate_loss)
            return None
        return mean_value_loss, mean_surrogate_loss

    def resolve(self):
        """The losses of an update(defer=True) (applying the fused path's learning-rate readback),
        or None when none is pending."""
        if self._fused is not None:
            return self._fused.resolve()
        out, self._deferred = self._deferred, None
        return out
