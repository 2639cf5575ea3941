"""rsl_rl 2.x `Distillation`: behaviour cloning of a privileged teacher into a student that reads the
deployable observations (DESIGN.md 4.3g has the semantics and the deviations).

The student acts in the env; every step stores the student's observation row and the teacher's
action mean for the same step's privileged row.  update() walks the T stored steps in order, sums
mean((student(obs_t) - teacher_t)^2) over `gradient_length` consecutive steps and takes one Adam
step per such chunk.  The teacher and `std` never change.

On a GPU the update runs on the lgx kernels (FusedDistillationUpdate, rl/fused_distillation.py)
when they take the policy and the chunk size; `use_fused_update=False`, a CPU device or an
unsupported shape runs the autograd update below, which is the reference path.  `fused` says which
one the last update() / chunk_gradient() ran.
"""
import torch
import torch.nn as nn
import torch.optim as optim
from torch.distributions import Normal

from .actor_critic import launch_forward, make_descs
from .fused import stream_of
from .fused_distillation import FusedDistillationUpdate
from .student_teacher import StudentTeacher


def _symmetry_on(cfg):
    if cfg is None:
        return False
    get = cfg.get if isinstance(cfg, dict) else lambda k, d=None: getattr(cfg, k, d)
    return bool(get("use_data_augmentation", False)) or bool(get("use_mirror_loss", False))


class DistillationStorage:
    """What an update reads: `observations` [T, N, W] and `privileged_actions` [T, N, A].  The
    observation rows are allocated with a row stride of W rounded up to 128 floats, the padding
    columns zero and never written (`padded` is the [T, N, stride] buffer): a chunk of consecutive
    steps is then directly a GEMM operand of the fused update, with no gather and no copy.  The
    privileged observations themselves are not stored (rsl_rl 2.x stores them and never reads them)."""

    ROW_PAD = 128

    def __init__(self, num_envs, num_transitions_per_env, num_obs, num_actions, device="cpu"):
        self.device = device
        self.num_envs, self.num_transitions_per_env = num_envs, num_transitions_per_env
        stride = -(-num_obs // self.ROW_PAD) * self.ROW_PAD
        self.padded = torch.zeros(num_transitions_per_env, num_envs, stride, device=device)
        self.observations = self.padded[..., :num_obs]
        self.privileged_actions = torch.zeros(num_transitions_per_env, num_envs, num_actions, device=device)
        self.step = 0

    def clear(self):
        self.step = 0


class Distillation:
    policy: StudentTeacher

    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None,
                 loss_type="mse", device="cpu", use_fused_update=True, symmetry=None):
        if getattr(policy, "is_recurrent", False):
            raise ValueError("Distillation: recurrent students are not supported (policy.is_recurrent)")
        if loss_type != "mse":
            raise ValueError(f"algorithm.loss_type = {loss_type!r}: only \"mse\" is implemented")
        if _symmetry_on(symmetry):
            raise ValueError("algorithm.symmetry is not supported with Distillation")
        if int(gradient_length) < 1 or int(num_learning_epochs) < 1:
            raise ValueError("algorithm.gradient_length and algorithm.num_learning_epochs must be >= 1")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("Distillation runs on one rank: the process group has "
                             f"{dist.get_world_size()} (multi-GPU distillation is not implemented)")
        self.device = device
        self.policy = self.actor_critic = policy.to(device)   # (OnPolicyRunner reaches it as actor_critic)
        self.num_learning_epochs = int(num_learning_epochs)
        self.gradient_length = int(gradient_length)
        self.learning_rate = learning_rate     # fixed: there is no schedule
        self.max_grad_norm = max_grad_norm
        self.loss_type = loss_type
        self.storage = None
        self.defer_store = False               # (OnPolicyRunner sets it; every store here is immediate)
        self.fused = False                     # which path the last update() / chunk_gradient() ran
        self._deferred = None
        self._fused = None
        cuda = str(device).startswith("cuda")
        params = list(policy.student.parameters()) + [policy.std]
        if cuda and use_fused_update and FusedDistillationUpdate.supported(policy):
            self._fused = FusedDistillationUpdate(self)   # student parameters + std become views of its flat buffer
            self.optimizer = self._fused.optimizer
        else:
            self.optimizer = optim.Adam(params, lr=learning_rate, fused=cuda or None)

    # ---------------------------------------------------------------- setup / modes
    def init_storage(self, num_envs, num_transitions_per_env, obs_shape, teacher_obs_shape, action_shape):
        """(OnPolicyRunner's call; teacher_obs_shape is unused: the privileged rows are not stored)"""
        if num_transitions_per_env % self.gradient_length:
            raise ValueError(f"runner.num_steps_per_env = {num_transitions_per_env} is not a multiple of "
                             f"algorithm.gradient_length = {self.gradient_length}: a chunk is gradient_length "
                             "contiguous steps of one rollout")
        self.storage = DistillationStorage(num_envs, num_transitions_per_env, obs_shape[0], action_shape[0], self.device)

    def test_mode(self):
        self.policy.eval()

    def train_mode(self):
        self.policy.train()

    def _need_teacher(self):
        if not self.policy.loaded_teacher:
            raise ValueError("Distillation: no teacher has been loaded (resume from a PPO checkpoint of a "
                             "privileged_actor run, or from a distillation checkpoint)")

    # ---------------------------------------------------------------- rollout
    def act(self, obs, teacher_obs):
        """The student's action sample for `obs`; stores `obs` and the teacher's action mean for
        `teacher_obs`.  On a GPU both networks run in one fused launch and the teacher's means land
        in the storage row directly."""
        self._need_teacher()
        st, policy = self.storage, self.policy
        s = st.step
        if s >= st.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        pair = policy.fused_pair(obs)
        if pair is not None:
            obs, teacher_obs = obs.contiguous(), teacher_obs.contiguous()
            mean = torch.empty(obs.shape[0], st.privileged_actions.shape[-1], device=obs.device)
            descs = make_descs([(pair[0], obs, mean), (pair[1], teacher_obs, st.privileged_actions[s])])
            launch_forward(descs, 2, stream_of(obs))
            policy.distribution = Normal(mean, mean * 0.0 + policy.std)
            actions = policy.distribution.sample()
        else:
            actions = policy.act(obs).detach()
            st.privileged_actions[s].copy_(policy.evaluate(teacher_obs))
        st.observations[s].copy_(obs)
        return actions

    def process_env_step(self, rewards, dones, infos):
        self.storage.step += 1
        self.policy.reset(dones)

    def compute_returns(self, last_obs):
        pass   # (no returns in behaviour cloning)

    def flush_store(self):
        pass

    def drop_store(self):
        pass

    # ---------------------------------------------------------------- update
    def _chunk_loss(self, c):
        """(autograd) the accumulated loss of chunk c and its per-step losses, detached"""
        st, g = self.storage, self.gradient_length
        loss, steps = 0.0, []
        for t in range(c * g, (c + 1) * g):
            l_t = nn.functional.mse_loss(self.policy.student(st.observations[t]), st.privileged_actions[t])
            loss = loss + l_t
            steps.append(l_t.detach())
        return loss, steps

    def _use_fused(self):
        M = self.gradient_length * self.storage.num_envs
        return self._fused is not None and FusedDistillationUpdate.supported(self.policy, M)

    def _student_grads(self):
        return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                          for p in self.policy.student.parameters()])

    def chunk_gradient(self, c):
        """d(chunk c's accumulated loss) / d(student parameters), flat in parameters() order, by the
        path an update would take now (`fused` says which); no optimizer step."""
        self._need_teacher()
        self.fused = self._use_fused()
        if self.fused:
            self._fused.gradients(c)
        else:
            self.optimizer.zero_grad()
            self._chunk_loss(c)[0].backward()
        return self._student_grads().clone()

    def update(self, defer=False):
        """rsl_rl Distillation.update -> the mean behaviour loss over epochs x steps.  defer=True
        issues the update and returns None; resolve() returns the loss later."""
        self._need_teacher()
        st = self.storage
        if st.step != st.num_transitions_per_env:
            raise ValueError(f"Distillation.update: the storage holds {st.step} of {st.num_transitions_per_env} steps")
        self.fused = self._use_fused()
        if self.fused:
            out = self._fused.update(defer=defer)
        else:
            total = 0.0
            student = list(self.policy.student.parameters())
            for _ in range(self.num_learning_epochs):
                for c in range(st.num_transitions_per_env // self.gradient_length):
                    loss, steps = self._chunk_loss(c)
                    total = total + sum(steps)
                    self.optimizer.zero_grad()
                    loss.backward()
                    if self._fused is not None:   # (parameters live in the flat buffer: its clip + Adam launch)
                        self._fused.step()
                        continue
                    if self.max_grad_norm:
                        nn.utils.clip_grad_norm_(student, self.max_grad_norm)
                    self.optimizer.step()
            out = (total / (self.num_learning_epochs * st.num_transitions_per_env)).item()
            if defer:
                self._deferred, out = out, None
        self.policy.invalidate_fused()
        st.clear()
        return out

    def resolve(self):
        """The loss of an update(defer=True), or None when none is pending."""
        if self._fused is not None and self._fused.pending:
            return self._fused.resolve()
        out, self._deferred = self._deferred, None
        return out
