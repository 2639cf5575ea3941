"""OnPolicyRunner with the rsl_rl v1.0.x contract consumed by the reference
(task_registry.py:159-167, train.py:43, play.py:65-71): `OnPolicyRunner(env, train_cfg_dict,
log_dir, device)`, `learn(num_learning_iterations, init_at_random_ep_len)`, `save`, `load`,
`get_inference_policy`, `alg.actor_critic`; checkpoint dict {model_state_dict,
optimizer_state_dict, iter, infos} saved every `save_interval` iterations as model_<it>.pt.

Timing: `collection_time` (act + env.step + storage) and `learn_time` (GAE + update) per
iteration, fps = num_steps_per_env * num_envs / (collection + learn), as rsl_rl logs it;
`last_iteration_stats` keeps them for bench.py.

`runner.empirical_normalization = True` (rsl_rl 2.x's key; off by default, and a dict without it is
off) puts an EmpiricalNormalization (rl/normalizer.py) in front of the actor and the critic:
`obs_normalizer` (env.num_obs wide) and `critic_obs_normalizer` (num_privileged_obs wide; the same
object when the env has no privileged row).  learn() normalises each step's rows right after
env.step, with an update; the storage, the returns and the update then see normalised rows.  The
checkpoint gains `obs_norm_state_dict` (and `critic_obs_norm_state_dict` for a separate critic
normaliser), and load() refuses a checkpoint from the other side of the flag.

`runner.privileged_actor = True` (read like empirical_normalization: a dict without it is off)
trains a teacher: the env's privileged row is the one observation row of actor and critic
(`ActorCritic(num_priv, num_priv, A)`, stored once), and get_inference_policy() expects that row.

`algorithm_class_name = "Distillation"` with `policy_class_name = "StudentTeacher"`
runs the same loop: the student acts on the env's observations, the teacher labels the privileged
row, `Loss/behavior` replaces the value and surrogate losses, and load() follows
StudentTeacher.load_state_dict: a PPO checkpoint only provides the teacher (iteration 0, fresh
optimizer), a distillation checkpoint resumes.
"""
import os
import statistics
import time

import torch

from .actor_critic import ActorCritic, ActorCriticRecurrent  # noqa: F401  (resolved by name from the cfg)
from .episode_stats import EpisodeStats
from .normalizer import EmpiricalNormalization, normalize_many
from .distillation import Distillation
from .ppo import PPO  # noqa: F401
from .student_teacher import StudentTeacher


class OnPolicyRunner:
    def __init__(self, env, train_cfg, log_dir=None, device="cpu"):
        self.cfg = train_cfg["runner"]
        self.alg_cfg = train_cfg["algorithm"]
        self.policy_cfg = train_cfg["policy"]
        self.device = device
        self.env = env
        num_critic_obs = self.env.num_privileged_obs if self.env.num_privileged_obs is not None else self.env.num_obs
        ac_class = {"ActorCritic": ActorCritic, "ActorCriticRecurrent": ActorCriticRecurrent,
                    "StudentTeacher": StudentTeacher}[self.cfg["policy_class_name"]]
        alg_class = {"PPO": PPO, "Distillation": Distillation}[self.cfg["algorithm_class_name"]]
        self.distillation = alg_class is Distillation
        # the privileged row as the env's one observation row (a teacher for Distillation)
        self.privileged_actor = bool(self.cfg.get("privileged_actor", False))
        num_actor_obs = self.env.num_obs
        if self.privileged_actor or self.distillation:
            self._check_teacher_student_cfg(ac_class)
        if self.privileged_actor:
            num_actor_obs = num_critic_obs
        actor_critic = ac_class(num_actor_obs, num_critic_obs, self.env.num_actions, **self.policy_cfg).to(self.device)
        self.alg = alg_class(actor_critic, device=self.device, **self.alg_cfg)
        if getattr(self.alg, "symmetry", False):   # algorithm.symmetry.use_data_augmentation / use_mirror_loss
            if self.cfg.get("empirical_normalization", False):
                raise ValueError("symmetry.use_data_augmentation / use_mirror_loss with runner.empirical_normalization: "
                                 "the storage holds normalised rows, and per-column statistics are not mirror-symmetric")
            self.alg.init_symmetry(self.env.symmetry_tables())
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]
        self.alg.init_storage(self.env.num_envs, self.num_steps_per_env, [num_actor_obs],
                              [None if self.privileged_actor else self.env.num_privileged_obs], [self.env.num_actions])
        self.obs_normalizer = self.critic_obs_normalizer = None
        if self.cfg.get("empirical_normalization", False):
            until = self.cfg.get("empirical_normalization_until")
            self.obs_normalizer = EmpiricalNormalization(self.env.num_obs, until=until, device=self.device)
            self.critic_obs_normalizer = self.obs_normalizer
            if self.env.num_privileged_obs is not None:
                self.critic_obs_normalizer = EmpiricalNormalization(num_critic_obs, until=until, device=self.device)
        self.log_dir = log_dir
        self.writer = None
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.last_iteration_stats = {}
        _, _ = self.env.reset()

    def _check_teacher_student_cfg(self, ac_class):
        """The refusals of runner.privileged_actor and of Distillation (each names its key)."""
        what = "runner.privileged_actor" if self.privileged_actor else "algorithm_class_name = \"Distillation\""
        if self.env.num_privileged_obs is None:
            raise ValueError(f"{what} needs an env with a privileged row (env.num_privileged_obs is None)")
        if self.cfg.get("empirical_normalization", False):
            raise ValueError(f"runner.empirical_normalization is not supported with {what}")
        if self.privileged_actor and self.distillation:
            raise ValueError("runner.privileged_actor trains a PPO teacher; Distillation reads the privileged row itself")
        if self.distillation != (ac_class is StudentTeacher):
            raise ValueError("algorithm_class_name = \"Distillation\" and policy_class_name = \"StudentTeacher\" "
                             "go together")
        if self.privileged_actor:
            sym = self.alg_cfg.get("symmetry") or {}
            if sym.get("use_data_augmentation", False) or sym.get("use_mirror_loss", False):
                raise ValueError("algorithm.symmetry is not supported with runner.privileged_actor (the observation "
                                 "table does not mirror the privileged row)")

    def _rows(self, obs, privileged_obs):
        """(actor rows, critic rows) of an env step: the observations and the privileged row (the
        observations again without one); runner.privileged_actor: the privileged row for both."""
        critic_obs = privileged_obs if privileged_obs is not None else obs
        return (critic_obs if self.privileged_actor else obs), critic_obs

    def _loss_locs(self, losses):
        """An update's result as log()'s entries: PPO's (mean value loss, mean surrogate loss), or
        Distillation's mean behaviour loss."""
        if self.distillation:
            return {"mean_behavior_loss": losses}
        return {"mean_value_loss": losses[0], "mean_surrogate_loss": losses[1]}

    def _writer(self):
        if self.writer is None and self.log_dir is not None:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
            except Exception:
                self.writer = False
        return self.writer or None

    def _normalize(self, obs, critic_obs, update=None):
        """(obs, critic_obs) through the normalisers (both in the same launches; one shared
        normaliser: applied once, the one result for actor and critic); as they are with the flag off."""
        nz, cz = self.obs_normalizer, self.critic_obs_normalizer
        if nz is None:
            return obs, critic_obs
        if cz is nz:
            y = nz(obs, update)
            return y, y
        return tuple(normalize_many([nz, cz], [obs, critic_obs], update))

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf,
                                                             high=int(self.env.max_episode_length))
        obs = self.env.get_observations()
        privileged_obs = self.env.get_privileged_observations()
        obs, critic_obs = self._rows(obs, privileged_obs)
        obs, critic_obs = obs.to(self.device), critic_obs.to(self.device)
        normalizing = self.obs_normalizer is not None
        if normalizing:
            # counted only by an empty normaliser: otherwise this row was the last one of the
            # previous learn() (or of the run the checkpoint came from) and is in the statistics
            obs, critic_obs = self._normalize(obs, critic_obs, update=self.obs_normalizer.count == 0)
        self.alg.actor_critic.train()
        ep_infos = []
        # Phase times on CUDA come from stream events read after update(), whose statistics readback
        # already waits for the stream: no extra host synchronisation between the rollout and the
        # update (upstream rsl_rl likewise times with time.time() and no sync).
        cuda = str(self.device).startswith("cuda")
        # Without a log directory nothing reads an iteration's statistics before the next one is
        # issued: the update is issued with a deferred readback and its statistics are taken once the
        # next rollout has been issued, so the GPU goes from the update straight into that rollout
        # (otherwise it idles ~0.3 ms per iteration while the host returns from the update's
        # synchronisation and issues again).  Same computation, same results.
        # With a log directory the update is synchronous and the iteration is logged at once.
        # LGX_DEFER_LOG=1 defers there too: iteration i is logged (same number, same values) once
        # rollout i + 1 has been issued; an iteration that writes a checkpoint stays synchronous, so
        # model_<it>.pt holds the parameters it always held.
        logged = self.log_dir is not None
        defer_log = cuda and logged and os.environ.get("LGX_DEFER_LOG", "0") == "1"
        pending = prev_end = None
        # Episode statistics (mean reward / length of the last 100 finished episodes): on CUDA one
        # lgx_episode_stats_step launch per env step and one readback per iteration, no host
        # synchronisation during collection; LGX_DEVICE_STATS=0 (and the CPU runner): rsl_rl's
        # torch / deque block, two blocking gathers per step.  Same lists either way.
        stats = EpisodeStats(self.env.num_envs, self.device, capacity=100,
                             kernel=cuda and os.environ.get("LGX_DEVICE_STATS", "1") != "0") if logged else None
        # act -> env.step -> process_env_step: each step's storage-row store rides on the next act's
        # launch (LGX_DEFER_STORE=0: its own launch, as before)
        self.alg.defer_store = os.environ.get("LGX_DEFER_STORE", "1") != "0"
        tot_iter = self.current_learning_iteration + num_learning_iterations
        completed = False
        try:
            for it in range(self.current_learning_iteration, tot_iter):
                start = time.time()
                defer = cuda and (not logged or (defer_log and it % self.save_interval != 0))
                if cuda:   # (the previous iteration's end event is this one's start: one marker less)
                    ev = [prev_end if prev_end is not None else torch.cuda.Event(enable_timing=True)] + \
                         [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    if prev_end is None:
                        ev[0].record()
                    prev_end = ev[2] if defer else None   # (synchronous runs: host logging lies between)
                with torch.inference_mode():
                    for _ in range(self.num_steps_per_env):
                        actions = self.alg.act(obs, critic_obs)
                        obs, privileged_obs, rewards, dones, infos = self.env.step(actions)
                        obs, critic_obs = self._rows(obs, privileged_obs)
                        obs, critic_obs = obs.to(self.device), critic_obs.to(self.device)
                        if normalizing:
                            obs, critic_obs = self._normalize(obs, critic_obs)
                        rewards, dones = rewards.to(self.device), dones.to(self.device)
                        self.alg.process_env_step(rewards, dones, infos)
                        if logged:
                            if "episode" in infos:
                                ep_infos.append(infos["episode"])
                            stats.step(rewards, dones)
                    ticket = stats.request() if logged else None   # (read in log(), after the update)
                    if cuda:
                        ev[1].record()
                    stop = time.time()
                    collection_time = stop - start
                    start = stop
                    self.alg.flush_store()           # (the last step's storage row: no act follows it)
                    self.alg.compute_returns(critic_obs)
                if pending is not None:
                    p, pending = pending, None
                    self._finish_deferred(p)
                if defer:
                    self.alg.update(defer=True)
                    ev[2].record()
                    pending = (ev, None)
                    if logged:   # what log() reads from the device, as it is after this update
                        pending = (ev, dict(it=it, num_learning_iterations=num_learning_iterations, ep_infos=ep_infos,
                                            stats=stats, ticket=ticket,
                                            device_values=self._log_values(ep_infos, defer=True)))
                        ep_infos = []
                    ep_infos.clear()
                    continue
                losses = self._loss_locs(self.alg.update())
                stop = time.time()
                learn_time = stop - start
                if cuda:
                    ev[2].record()
                    ev[2].synchronize()
                    collection_time = ev[0].elapsed_time(ev[1]) * 1e-3
                    learn_time = ev[1].elapsed_time(ev[2]) * 1e-3
                self.last_iteration_stats = dict(collection_time=collection_time, learn_time=learn_time,
                                                 **{k[len("mean_"):]: v for k, v in losses.items()},
                                                 learning_rate=self.alg.learning_rate, **self._symmetry_stats())
                if logged:
                    rewbuffer, lenbuffer = stats.result(ticket)
                    self.log(dict(it=it, num_learning_iterations=num_learning_iterations, ep_infos=ep_infos,
                                  collection_time=collection_time, learn_time=learn_time, **losses,
                                  rewbuffer=rewbuffer, lenbuffer=lenbuffer, **self._symmetry_stats()))
                    if it % self.save_interval == 0:
                        self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
                ep_infos.clear()
            completed = True
        finally:
            # also on an exception: no deferred storage row may outlive learn() holding pointers to
            # the env's reward / reset / time-out buffers (the env has not stepped since that row's
            # process_env_step: every env.step follows an act, which takes the pending row), and no
            # update readback stays pending.  While an exception propagates (possibly a GPU error,
            # which the cleanup's launches and synchronisation would raise again) the cleanup is
            # best-effort and the original exception is the one reported.
            self.alg.defer_store = False
            p, pending = pending, None
            try:
                self.alg.flush_store()
                if p is not None:
                    self._finish_deferred(p, log=completed)
            except Exception:
                if completed:
                    raise
                self.alg.drop_store()
        self.current_learning_iteration += num_learning_iterations
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    def _finish_deferred(self, pending, log=True):
        """Statistics of a deferred iteration: losses and learning rate from the update's readback,
        phase times from its stream events (all complete by the time the next rollout is issued);
        then its log entry (LGX_DEFER_LOG=1)."""
        ev, locs = pending
        losses = self._loss_locs(self.alg.resolve())
        ev[2].synchronize()
        self.last_iteration_stats = dict(collection_time=ev[0].elapsed_time(ev[1]) * 1e-3,
                                         learn_time=ev[1].elapsed_time(ev[2]) * 1e-3,
                                         **{k[len("mean_"):]: v for k, v in losses.items()},
                                         learning_rate=self.alg.learning_rate, **self._symmetry_stats())
        if locs is not None and log:
            rewbuffer, lenbuffer = locs.pop("stats").result(locs.pop("ticket"))
            self.log(dict(locs, collection_time=self.last_iteration_stats["collection_time"],
                          learn_time=self.last_iteration_stats["learn_time"], **losses, rewbuffer=rewbuffer,
                          lenbuffer=lenbuffer,
                          **self._symmetry_stats()))

    def _symmetry_stats(self):
        """{"symmetry_loss": the last (resolved) update's mean symmetry loss} with the mirror loss on, else {}."""
        if getattr(self.alg, "mirror_loss_coeff", None) is None:
            return {}
        return {"symmetry_loss": self.alg.symmetry_loss}

    def _log_values(self, ep_infos, defer=False):
        """What log() reads from the device, in one reduction and one readback: the mean over the
        rollout's steps of every extras["episode"] scalar (in key order), then the mean action noise
        std.  defer=True: (pinned host tensor, event) of a non-blocking copy instead of the list."""
        with torch.no_grad():
            vals = self.alg.actor_critic.std.detach().mean().reshape(1)
            if ep_infos:
                keys = list(ep_infos[0])
                steps = torch.stack([torch.as_tensor(ep[key], device=self.device).reshape(())
                                     for ep in ep_infos for key in keys]).float()
                vals = torch.cat([steps.view(len(ep_infos), len(keys)).mean(0), vals])
            if not defer:
                return vals.tolist()
            host = torch.empty(vals.shape, dtype=vals.dtype, pin_memory=True)
            host.copy_(vals, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            return host, event

    def log(self, locs, width=80, pad=35):
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
        self.tot_time += locs["collection_time"] + locs["learn_time"]
        it_time = locs["collection_time"] + locs["learn_time"]
        w = self._writer()
        lines = []
        values = locs.get("device_values")
        if values is None:
            values = self._log_values(locs["ep_infos"])
        elif not isinstance(values, list):
            values[1].synchronize()
            values = values[0].tolist()
        noise_std = values[-1]
        if locs["ep_infos"]:
            for key, value in zip(locs["ep_infos"][0], values):
                if w:
                    w.add_scalar("Episode/" + key, value, locs["it"])
                lines.append(f"{'Mean episode ' + key + ':':>{pad}} {value:.4f}")
        fps = int(self.num_steps_per_env * self.env.num_envs / it_time)
        if w:
            if "mean_behavior_loss" in locs:
                w.add_scalar("Loss/behavior", locs["mean_behavior_loss"], locs["it"])
            else:
                w.add_scalar("Loss/value_function", locs["mean_value_loss"], locs["it"])
                w.add_scalar("Loss/surrogate", locs["mean_surrogate_loss"], locs["it"])
            if "symmetry_loss" in locs:
                w.add_scalar("Loss/symmetry", locs["symmetry_loss"], locs["it"])
            w.add_scalar("Loss/learning_rate", self.alg.learning_rate, locs["it"])
            w.add_scalar("Policy/mean_noise_std", noise_std, locs["it"])
            w.add_scalar("Perf/total_fps", fps, locs["it"])
            w.add_scalar("Perf/collection time", locs["collection_time"], locs["it"])
            w.add_scalar("Perf/learning_time", locs["learn_time"], locs["it"])
        header = f" \033[1m Learning iteration {locs['it']}/{self.current_learning_iteration + locs['num_learning_iterations']} \033[0m "
        s = f"{'#' * width}\n{header.center(width, ' ')}\n\n"
        s += f"{'Computation:':>{pad}} {fps:.0f} steps/s (collection: {locs['collection_time']:.3f}s, learning {locs['learn_time']:.3f}s)\n"
        if "mean_behavior_loss" in locs:
            s += f"{'Behavior loss:':>{pad}} {locs['mean_behavior_loss']:.4f}\n"
        else:
            s += f"{'Value function loss:':>{pad}} {locs['mean_value_loss']:.4f}\n"
            s += f"{'Surrogate loss:':>{pad}} {locs['mean_surrogate_loss']:.4f}\n"
        if "symmetry_loss" in locs:
            s += f"{'Symmetry loss:':>{pad}} {locs['symmetry_loss']:.4f}\n"
        s += f"{'Mean action noise std:':>{pad}} {noise_std:.2f}\n"
        if len(locs["rewbuffer"]) > 0:
            s += f"{'Mean reward:':>{pad}} {statistics.mean(locs['rewbuffer']):.2f}\n"
            s += f"{'Mean episode length:':>{pad}} {statistics.mean(locs['lenbuffer']):.2f}\n"
        s += "\n".join(lines) + "\n" + "-" * width + "\n"
        s += f"{'Total timesteps:':>{pad}} {self.tot_timesteps}\n{'Iteration time:':>{pad}} {it_time:.2f}s\n"
        print(s)

    def save(self, path, infos=None):
        d = {"model_state_dict": self.alg.actor_critic.state_dict(),
             "optimizer_state_dict": self.alg.optimizer.state_dict(),
             "iter": self.current_learning_iteration, "infos": infos}
        if self.obs_normalizer is not None:
            d["obs_norm_state_dict"] = self.obs_normalizer.state_dict()
            if self.critic_obs_normalizer is not self.obs_normalizer:
                d["critic_obs_norm_state_dict"] = self.critic_obs_normalizer.state_dict()
        torch.save(d, path)

    def load(self, path, load_optimizer=True):
        d = torch.load(path, map_location=self.device, weights_only=True)
        # a policy must not run on the wrong side of its normaliser
        has = "obs_norm_state_dict" in d or "critic_obs_norm_state_dict" in d
        if self.obs_normalizer is None and has:
            raise ValueError(f"{path} holds observation-normaliser statistics, but this runner has "
                             "runner.empirical_normalization off")
        if self.obs_normalizer is not None:
            separate = self.critic_obs_normalizer is not self.obs_normalizer
            if "obs_norm_state_dict" not in d or (separate and "critic_obs_norm_state_dict" not in d):
                raise ValueError(f"{path} holds no observation-normaliser statistics, but this runner has "
                                 "runner.empirical_normalization on")
            self.obs_normalizer.load_state_dict(d["obs_norm_state_dict"])
            if separate:
                self.critic_obs_normalizer.load_state_dict(d["critic_obs_norm_state_dict"])
        resumed = self.alg.actor_critic.load_state_dict(d["model_state_dict"])
        if hasattr(self.alg.actor_critic, "invalidate_fused"):
            self.alg.actor_critic.invalidate_fused()
        if resumed is False:   # StudentTeacher took a PPO checkpoint's actor as its teacher: not a resumed run
            return d["infos"]
        if load_optimizer:
            # as upstream rsl_rl: the optimizer state (its param_groups' lr included) is restored and
            # alg.learning_rate keeps the config value - the adaptive schedule's first update then
            # adapts from the config value and overwrites the restored lr, a fixed schedule steps
            # with the restored lr (tests/test_ppo.py::test_resume_learning_rate_follows_upstream)
            self.alg.optimizer.load_state_dict(d["optimizer_state_dict"])
        self.current_learning_iteration = d["iter"]
        return d["infos"]

    def get_inference_policy(self, device=None):
        """The deployable policy: observations -> action means.  runner.privileged_actor: it expects
        the env's privileged row (env.get_privileged_observations()); Distillation: the student."""
        self.alg.actor_critic.eval()
        if device is not None:
            self.alg.actor_critic.to(device)
        act_inference = self.alg.actor_critic.act_inference
        if self.obs_normalizer is None:
            return act_inference
        nz = self.obs_normalizer if device is None else self.obs_normalizer.to(device)

        def policy(obs):   # the frozen normaliser, then the actor: the statistics stay as they are
            return act_inference(nz(obs, update=False))
        return policy

    def close(self):
        """Release the update's collective resources (the lgx RCCL communicator of
        LGX_NATIVE_ALLREDUCE=1; collective: every rank calls it after its last learn())."""
        fused = getattr(self.alg, "_fused", None)
        if fused is not None:
            fused.close_comm()
