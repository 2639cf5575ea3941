"""The rollout's kernel driver, the counterpart of FusedPPOUpdate: PPO.act and
PPO.process_env_step on the lgx kernels, which write the storage rows themselves."""
import ctypes as C
import os

import torch

from legged_gym_amd.sim import abi
from legged_gym_amd.sim import lib as lgxlib

from .actor_critic import launch_forward, make_descs
from .fused import stream_of


def _switches():
    """(the fused act launch is allowed, the noise is drawn once per rollout): the module's only
    reader of os.environ, taken once when the driver is built."""
    return os.environ.get("LGX_FUSED_ACT", "1") != "0", os.environ.get("LGX_BATCHED_NOISE", "0") == "1"


class FusedRollout:
    @staticmethod
    def supported(ac):
        # (per call besides: GPU observations, room in the storage, no autograd, use_fused_inference)
        return not ac.is_recurrent and ac.heads_fused

    def __init__(self, ppo, lib):
        self.ppo, self.lib = ppo, lib
        self.fused_act, self.batched_noise = _switches()
        self.mean = self.actions = self.noise = None   # the act launch's [N, A] outputs, and the draws it reads
        self.pending = None               # deferred store: (LgxPpoStoreArgs, the tensors it points into...)
        self.fused_off = False            # the fused act launch refused this network pair: two launches from now on
        self.last_fused = False           # the last act was the single fused launch

    def act(self, obs, critic_obs):
        """The actions, their storage rows written (+ the previous step's deferred store) in ONE launch, or
        None when the kernels do not take this call.  lgx_mlp_x3_forward_act runs the actor and critic
        MLPs and lgx_ppo_act's arithmetic in the actor's last-layer epilogue (the critic writes its
        storage row directly).  Switched off, or a network pair the fused launch does not take: the MLP
        launch, then lgx_ppo_act(_store) - bit-identical rows either way."""
        ppo, st = self.ppo, self.ppo.storage
        room = st is not None and st.step < st.num_transitions_per_env
        heads = ppo.actor_critic.fused_heads(obs) if room else None   # (None as well for CPU observations)
        if heads is None:
            return None
        s, T = st.step, st.num_transitions_per_env
        obs, critic_obs = obs.contiguous(), critic_obs.contiguous()
        shape = (obs.shape[0], heads[0].dims[-1])
        if self.mean is None or self.mean.shape != shape:
            self.mean = torch.empty(shape, device=obs.device)
            self.actions = torch.empty_like(self.mean)
        descs = make_descs([(heads[0], obs, self.mean), (heads[1], critic_obs, st.values[s])])
        # Normal.sample's standard-normal draws from torch's generator.  Default: one [N, A] draw per step,
        # the RNG consumption of rsl_rl's Normal.sample (torch.normal(mu, std) = normal_(0, 1) * std + mu),
        # so seeded runs draw the same noise as upstream.  Batched: one [T, N, A] draw per rollout (one
        # launch instead of T; same distribution, different RNG stream, T*N*A floats kept)
        if not self.batched_noise:
            noise = self.noise = torch.randn(shape, device=obs.device)   # (kept alive until the kernel has read it)
        else:
            if s == 0 or self.noise is None or self.noise.shape != (T,) + shape:
                self.noise = torch.randn((T,) + shape, device=obs.device)
            noise = self.noise[s]
        a = abi.LgxPpoActArgs()
        a.num_envs, a.num_actions, a.num_obs = shape[0], shape[1], obs.shape[1]
        a.mu, a.value, a.std, a.noise = self.mean.data_ptr(), None, ppo.actor_critic.std.data_ptr(), noise.data_ptr()
        if st.privileged_observations is not None:
            a.num_cobs, a.cobs, a.st_cobs = critic_obs.shape[1], critic_obs.data_ptr(), \
                st.privileged_observations[s].data_ptr()
        a.obs, a.actions_out = obs.data_ptr(), self.actions.data_ptr()
        a.st_obs, a.st_actions, a.st_values = st.observations[s].data_ptr(), st.actions[s].data_ptr(), \
            st.values[s].data_ptr()
        a.st_logp, a.st_mu, a.st_sigma = st.actions_log_prob[s].data_ptr(), st.mu[s].data_ptr(), st.sigma[s].data_ptr()
        lib, stream = self.lib, stream_of(obs)
        prev = self.pending[0] if self.pending is not None and self.pending[0].num_envs == a.num_envs else None
        if prev is None:
            self.flush()
        fused = isinstance(descs[0], abi.LgxMlpX3Desc) and self.fused_act and not self.fused_off
        if fused and lib.lgx_mlp_x3_forward_act(descs, 2, C.byref(a), C.byref(prev) if prev is not None else None,
                                                stream) != 0:
            # (validated before any launch) a pair the fused launch does not take, e.g. the act
            # rows past the LDS: the two-launch form from now on
            self.fused_off, fused = True, False
        if not fused:
            launch_forward(descs, 2, stream)   # actor and critic in one launch
            if prev is not None:   # the previous step's store rides along
                lgxlib.check(lib.lgx_ppo_act_store(C.byref(a), C.byref(prev), stream), "lgx_ppo_act_store")
            else:
                lgxlib.check(lib.lgx_ppo_act(C.byref(a), stream), "lgx_ppo_act")
        self.last_fused, self.pending = fused, None   # (prev, if any, has been launched)
        t = ppo.transition
        t.actions, t.values = self.actions, st.values[s]
        t.actions_log_prob, t.action_mean, t.action_sigma = st.actions_log_prob[s], st.mu[s], st.sigma[s]
        t.observations, t.critic_observations = obs, critic_obs
        t.in_storage = True
        return self.actions

    def store(self, rewards, dones, infos):
        """The reward / done rows of the step whose other rows act() wrote (lgx_ppo_store)."""
        st = self.ppo.storage
        a = abi.LgxPpoStoreArgs()
        rewards, dones = rewards.contiguous(), dones.contiguous()
        a.num_envs, a.gamma, a.rew, a.reset = st.num_envs, self.ppo.gamma, rewards.data_ptr(), dones.data_ptr()
        to = infos.get("time_outs") if isinstance(infos, dict) else None
        if to is not None:
            to = to.contiguous()
            a.time_outs = to.data_ptr()
        a.st_values, a.st_rew, a.st_dones = st.values[st.step].data_ptr(), st.rewards[st.step].data_ptr(), \
            st.dones[st.step].data_ptr()
        # PPO.defer_store: launched with the next act (lgx_ppo_act_store) or by flush(): the env's
        # reward / reset / time-out buffers hold this step's values until the next env.step, which
        # the runner issues only after that act
        self.flush()
        self.pending = (a, rewards, dones, to)
        if not self.ppo.defer_store:
            self.flush()

    def flush(self):
        """Launch a deferred lgx_ppo_store on its own."""
        pend, self.pending = self.pending, None
        if pend is not None:
            lgxlib.check(self.lib.lgx_ppo_store(C.byref(pend[0]), stream_of(pend[1])), "lgx_ppo_store")

    def drop(self):
        """Forget a deferred row without launching it."""
        self.pending = None
