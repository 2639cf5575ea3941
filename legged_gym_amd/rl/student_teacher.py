"""rsl_rl 2.x `StudentTeacher`: the policy pair of teacher-student distillation.

`student` reads the env's observation row and is what trains and deploys; `teacher` reads the
privileged row, comes from a PPO checkpoint's actor (a `privileged_actor` run, task
go1_rough_teacher), is always in eval mode and never receives a gradient.  The no-grad forwards of
both run on the fused MLP kernels (_FusedMLP), as ActorCritic's do; `Distillation.act` puts the
two into one launch.
"""
import torch
import torch.nn as nn
from torch.distributions import Normal

from .actor_critic import _FusedMLP, _mlp, get_activation


class StudentTeacher(nn.Module):
    is_recurrent = False

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims=(256, 256, 256),
                 teacher_hidden_dims=(256, 256, 256), activation="elu", init_noise_std=0.1, **kwargs):
        recurrent = sorted(k for k in kwargs if k.startswith("rnn_"))
        if recurrent:
            raise ValueError(f"StudentTeacher: recurrent students are not supported (policy key(s) {recurrent})")
        if kwargs:
            print("StudentTeacher.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs.keys())))
        super().__init__()
        act = get_activation(activation)
        self.loaded_teacher = False
        self.student = _mlp(num_student_obs, list(student_hidden_dims), num_actions, act)
        self.teacher = _mlp(num_teacher_obs, list(teacher_hidden_dims), num_actions, act)
        self.teacher.eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        print(f"Student MLP: {self.student}")
        print(f"Teacher MLP: {self.teacher}")
        self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        self.distribution = None
        Normal.set_default_validate_args(False)
        self._fused_student = _FusedMLP(self.student)
        self._fused_teacher = _FusedMLP(self.teacher)
        self.use_fused_inference = True

    def reset(self, dones=None):
        pass

    def forward(self):
        raise NotImplementedError

    def train(self, mode=True):
        super().train(mode)
        self.teacher.eval()   # (the teacher is always in eval mode)
        return self

    def invalidate_fused(self):
        """Call after parameters change outside autograd-visible in-place ops (optimizer step, load)."""
        self._fused_student.invalidate()
        self._fused_teacher.invalidate()

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    def _fused_ok(self, x, fused):
        return (self.use_fused_inference and fused.ok and x.is_cuda and
                (torch.is_inference_mode_enabled() or not torch.is_grad_enabled()))

    def fused_pair(self, x):
        """(student, teacher) fused MLPs when one fused launch takes both for the student input `x` now, else None."""
        ok = self._fused_teacher.ok and self._fused_ok(x, self._fused_student)
        return (self._fused_student, self._fused_teacher) if ok else None

    def _student_mean(self, observations):
        if self._fused_ok(observations, self._fused_student):
            return self._fused_student(observations)
        return self.student(observations)

    def update_distribution(self, observations):
        mean = self._student_mean(observations)
        self.distribution = Normal(mean, mean * 0.0 + self.std)

    def act(self, observations, **kwargs):
        self.update_distribution(observations)
        return self.distribution.sample()

    def act_inference(self, observations):
        return self._student_mean(observations)

    def evaluate(self, teacher_observations, **kwargs):
        with torch.no_grad():
            if self._fused_ok(teacher_observations, self._fused_teacher):
                return self._fused_teacher(teacher_observations)
            return self.teacher(teacher_observations)

    def load_state_dict(self, state_dict, strict=True):
        """A PPO checkpoint (some key starts with `actor.`): its actor becomes the teacher, nothing
        else changes, returns False - not a resumed run.  A distillation checkpoint (`student.*` /
        `teacher.*` / `std`): everything is loaded, returns True."""
        if any(k.startswith("actor.") for k in state_dict):
            teacher = {k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
            self._check_teacher(teacher)
            self.teacher.load_state_dict(teacher, strict=True)
            resumed = False
        elif any(k.startswith("student.") for k in state_dict):
            self._check_teacher({k[len("teacher."):]: v for k, v in state_dict.items() if k.startswith("teacher.")})
            super().load_state_dict(state_dict, strict=True)
            resumed = True
        else:
            raise ValueError("StudentTeacher.load_state_dict: neither a PPO checkpoint (actor.*) nor a distillation "
                             "checkpoint (student.* / teacher.*)")
        self.loaded_teacher = True
        self.teacher.eval()
        self.invalidate_fused()
        return resumed

    def _check_teacher(self, teacher):
        """ValueError when the checkpoint's teacher reads or writes another width than this one
        (the env's num_privileged_obs in, num_actions out)."""
        linears = [m for m in self.teacher if isinstance(m, nn.Linear)]
        first, last = "0.weight", f"{len(self.teacher) - 1}.weight"
        if first in teacher and teacher[first].shape[1] != linears[0].in_features:
            raise ValueError(f"the checkpoint's teacher reads {teacher[first].shape[1]} inputs, this env's privileged "
                             f"row (env.num_privileged_obs) has {linears[0].in_features}")
        if last in teacher and teacher[last].shape[0] != linears[-1].out_features:
            raise ValueError(f"the checkpoint's teacher writes {teacher[last].shape[0]} actions, this env has "
                             f"num_actions = {linears[-1].out_features}")
