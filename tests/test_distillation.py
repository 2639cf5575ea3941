"""CPU: teacher-student distillation (rsl_rl 2.x Distillation + StudentTeacher) and the
runner.privileged_actor teacher: checkpoint loading, every refusal, the autograd update against the
float64 statement of tests/distillation_ref.py, and the runner plumbing that runs without a GPU (on a
stand-in env: the CPU oracle has no privileged row).

Gradient tolerance: |d| <= 1e-5 + 2e-3 |g|, as tests/test_gpu_symmetry.py.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import distillation_ref as ref
from legged_gym_amd.rl.distillation import Distillation
from legged_gym_amd.rl.student_teacher import StudentTeacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, G, W, P, A = 8, 4, 2, 20, 9, 12       # envs, steps, gradient_length, student / teacher widths, actions
HID = [128, 128]


def close(a, b, what):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    err = (a - b).abs()
    assert (err <= 1e-5 + 2e-3 * b.abs()).all(), (what, err.max().item(), b.abs().max().item())


def make_alg(epochs=2, max_grad_norm=None, seed=0, load_teacher=True, **kw):
    torch.manual_seed(seed)
    policy = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32], activation="elu")
    alg = Distillation(policy, num_learning_epochs=epochs, gradient_length=G, learning_rate=1e-3,
                       max_grad_norm=max_grad_norm, device="cpu", **kw)
    alg.init_storage(N, T, [W], [P], [A])
    if load_teacher:
        policy.loaded_teacher = True
    return alg


def fill(alg, seed=1):
    """A rollout's worth of act() calls on fixed rows; -> (obs [T, N, W], teacher obs [T, N, P])"""
    g = torch.Generator().manual_seed(seed)
    obs, tobs = torch.randn(T, N, W, generator=g), torch.randn(T, N, P, generator=g)
    for t in range(T):
        alg.act(obs[t], tobs[t])
        alg.process_env_step(None, torch.zeros(N, dtype=torch.bool), {})
    return obs, tobs


def student_params(policy):
    lin = [m for m in policy.student if isinstance(m, torch.nn.Linear)]
    return [(l.weight.detach().double().numpy().copy(), l.bias.detach().double().numpy().copy()) for l in lin]


# ---------------------------------------------------------------- the policy
def test_student_teacher_semantics():
    torch.manual_seed(0)
    p = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32], init_noise_std=0.1)
    assert not p.is_recurrent and not p.loaded_teacher
    assert p.std.shape == (A,) and torch.all(p.std == 0.1)
    p.train()
    assert p.student.training and not p.teacher.training             # the teacher is always in eval mode
    assert not any(q.requires_grad for q in p.teacher.parameters())
    x, y = torch.randn(5, W), torch.randn(5, P)
    assert torch.equal(p.act_inference(x), p.student(x))
    out = p.evaluate(y)
    assert torch.equal(out, p.teacher(y)) and not out.requires_grad
    torch.manual_seed(3)
    a = p.act(x)
    torch.manual_seed(3)
    assert torch.equal(a, torch.distributions.Normal(p.student(x), p.std.expand(5, A)).sample())
    with pytest.raises(ValueError, match="rnn_type"):
        StudentTeacher(W, P, A, rnn_type="lstm")


def test_load_state_dict_takes_a_ppo_checkpoint_as_the_teacher():
    from legged_gym_amd.rl.actor_critic import ActorCritic
    torch.manual_seed(0)
    ac = ActorCritic(P, P, A, actor_hidden_dims=[32], critic_hidden_dims=[16])
    p = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32])
    before = copy.deepcopy(p.state_dict())
    assert p.load_state_dict(ac.state_dict()) is False and p.loaded_teacher
    for k, v in ac.actor.state_dict().items():
        assert torch.equal(p.teacher.state_dict()[k], v), k
    for k, v in p.state_dict().items():                              # student and std keep their initial values
        if not k.startswith("teacher."):
            assert torch.equal(v, before[k]), k
    # a distillation checkpoint: everything, strictly
    q = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32])
    assert q.load_state_dict(p.state_dict()) is True and q.loaded_teacher
    for k, v in p.state_dict().items():
        assert torch.equal(q.state_dict()[k], v), k
    sd = p.state_dict()
    del sd["std"]
    with pytest.raises(RuntimeError):
        StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32]).load_state_dict(sd)
    with pytest.raises(ValueError, match="neither"):
        q.load_state_dict({"foo.weight": torch.zeros(1)})


def test_a_teacher_of_the_wrong_width_is_refused():
    from legged_gym_amd.rl.actor_critic import ActorCritic
    p = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32])
    with pytest.raises(ValueError, match="num_privileged_obs"):
        p.load_state_dict(ActorCritic(P + 1, P + 1, A, actor_hidden_dims=[32], critic_hidden_dims=[16]).state_dict())
    with pytest.raises(ValueError, match="num_actions"):
        p.load_state_dict(ActorCritic(P, P, A - 1, actor_hidden_dims=[32], critic_hidden_dims=[16]).state_dict())
    assert not p.loaded_teacher
    wide = StudentTeacher(W, P + 1, A, student_hidden_dims=HID, teacher_hidden_dims=[32])
    with pytest.raises(ValueError, match="num_privileged_obs"):
        p.load_state_dict(wide.state_dict())


# ---------------------------------------------------------------- the algorithm's refusals
def test_training_without_a_teacher_raises():
    alg = make_alg(load_teacher=False)
    with pytest.raises(ValueError, match="no teacher"):
        alg.act(torch.zeros(N, W), torch.zeros(N, P))
    with pytest.raises(ValueError, match="no teacher"):
        alg.update()


def test_refusals_name_their_key(monkeypatch):
    policy = StudentTeacher(W, P, A, student_hidden_dims=HID, teacher_hidden_dims=[32])
    with pytest.raises(ValueError, match="loss_type"):
        Distillation(policy, loss_type="huber")
    with pytest.raises(ValueError, match="algorithm.symmetry"):
        Distillation(policy, symmetry={"use_data_augmentation": True})
    with pytest.raises(ValueError, match="algorithm.symmetry"):
        Distillation(policy, symmetry={"use_mirror_loss": True, "mirror_loss_coeff": 1.0})
    Distillation(policy, symmetry={"use_data_augmentation": False})       # off is off
    alg = Distillation(policy, gradient_length=3)
    with pytest.raises(ValueError, match="gradient_length"):
        alg.init_storage(N, 4, [W], [P], [A])

    class Recurrent(StudentTeacher):
        is_recurrent = True
    with pytest.raises(ValueError, match="recurrent"):
        Distillation(Recurrent(W, P, A))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="one rank"):
        Distillation(policy)


# ---------------------------------------------------------------- the autograd update against float64
def test_rollout_stores_observations_and_teacher_means():
    alg = make_alg()
    obs, tobs = fill(alg)
    st = alg.storage
    assert st.observations.shape == (T, N, W) and st.privileged_actions.shape == (T, N, A)
    assert torch.equal(st.observations, obs)
    assert torch.equal(st.privileged_actions, alg.policy.teacher(tobs.view(T * N, P)).view(T, N, A).detach())
    assert st.padded.shape[-1] == 128 and torch.all(st.padded[..., W:] == 0)   # row stride: W rounded up to 128
    with pytest.raises(AssertionError, match="overflow"):
        alg.act(obs[0], tobs[0])


def test_chunk_gradient_matches_float64():
    alg = make_alg()
    obs, _ = fill(alg)
    target = alg.storage.privileged_actions.double().numpy()
    for c in range(T // G):
        g = alg.chunk_gradient(c)
        assert alg.fused is False
        _, _, grads = ref.chunk_loss_grad(student_params(alg.policy), obs[c * G:(c + 1) * G].double().numpy(),
                                          target[c * G:(c + 1) * G])
        want = np.concatenate([np.concatenate([gw.reshape(-1), gb.reshape(-1)]) for gw, gb in grads])
        close(g, want, f"chunk {c}")


@pytest.mark.parametrize("max_grad_norm", [None, 0.05], ids=["noclip", "clip"])
def test_update_matches_float64(max_grad_norm):
    """N = 8, T = 4, gradient_length = 2, 2 epochs, student 20 -> 128 -> 128 -> 12: four Adam steps.
    A parameter moves by about lr per step, whatever its gradient; two paths whose gradients agree to
    2e-3 relative give steps that agree to a like fraction of lr (1e-3), so the parameters are held
    to 1e-5 + 2e-3 of the distance they moved in all."""
    alg = make_alg(max_grad_norm=max_grad_norm)
    obs, _ = fill(alg)
    target = alg.storage.privileged_actions.double().numpy()
    p0 = student_params(alg.policy)
    teacher0, std0 = copy.deepcopy(alg.policy.teacher.state_dict()), alg.policy.std.detach().clone()
    loss = alg.update()
    assert alg.fused is False and alg.storage.step == 0
    want, want_loss = ref.update(p0, obs.double().numpy(), target, G, 2, 1e-3, max_grad_norm)
    assert abs(loss - want_loss) <= 1e-4 * abs(want_loss)
    for (W0, b0), (Ww, bw), (Wg, bg) in zip(p0, want, student_params(alg.policy)):
        for a0, w, g in ((W0, Ww, Wg), (b0, bw, bg)):
            assert (np.abs(g - w) <= 1e-5 + 2e-3 * np.abs(w - a0)).all(), np.abs(g - w).max()
            assert np.abs(w - a0).max() > 1e-4                                 # the update moved them
    # the teacher and std come out bit-identical
    for k, v in alg.policy.teacher.state_dict().items():
        assert torch.equal(v, teacher0[k]), k
    assert torch.equal(alg.policy.std.detach(), std0)


def test_behaviour_loss_falls_on_a_fixed_batch():
    alg = make_alg(epochs=1)
    losses = []
    for _ in range(3):
        fill(alg)                                   # the same rows every time
        losses.append(alg.update())
    assert losses[0] > losses[1] > losses[2] > 0, losses


def test_deferred_update_resolves_to_the_same_loss():
    a, b = make_alg(), make_alg()
    fill(a), fill(b)
    assert b.update(defer=True) is None
    assert b.resolve() == a.update() and b.resolve() is None


# ---------------------------------------------------------------- the library's entry points (host checks)
def test_entry_points_validate_without_a_gpu():
    import torch  # noqa: F401  (HIP runtime first)
    from legged_gym_amd.sim import abi
    lib = abi.declare(C.CDLL(os.path.join(ROOT, "legged_gym_amd", "liblgx.so")))
    lay = (C.c_int64 * 3)()
    assert lib.lgx_bc_loss_bwd_layout(37, 12, 128, lay) == 0
    assert tuple(lay) == (2, 2 * (12 * 128 + 12 + 128), (32 * 132 + 12 * 128 + 32 * 16 + 32) * 4)
    for bad in ((0, 12, 128), (37, 0, 128), (37, 17, 128), (37, 12, 120), (37, 12, 0), (37, 12, 1024)):
        assert lib.lgx_bc_loss_bwd_layout(*bad, lay) == -1, bad
        assert b"lgx_bc_loss_bwd_layout" in lib.lgx_last_error()
    p = C.c_void_p(0x1000)
    assert lib.lgx_bc_loss_bwd(None, p, p, p, 32, 12, 128, 1.0, p, p, None) == -1
    assert b"null pointer" in lib.lgx_last_error()
    assert lib.lgx_bc_loss_bwd(p, p, p, p, 32, 12, 128, float("nan"), p, p, None) == -1
    assert b"finite" in lib.lgx_last_error()
    assert lib.lgx_bc_loss_reduce(None, 4, 1.0, p, None) == -1
    assert lib.lgx_bc_loss_reduce(p, 0, 1.0, p, None) == -1


# ---------------------------------------------------------------- configs and the runner
class StandInEnv:
    """What OnPolicyRunner touches, with a privileged row (the CPU oracle cannot bind one)."""

    def __init__(self, num_obs=W, num_privileged_obs=P, seed=0):
        self.num_envs, self.num_obs, self.num_privileged_obs, self.num_actions = N, num_obs, num_privileged_obs, A
        self.max_episode_length = 100
        self.episode_length_buf = torch.zeros(N, dtype=torch.long)
        self.gen = torch.Generator().manual_seed(seed)
        self.actions = []
        self._draw()

    def _draw(self):
        self.obs = torch.randn(N, self.num_obs, generator=self.gen)
        self.priv = None if self.num_privileged_obs is None else torch.randn(N, self.num_privileged_obs,
                                                                             generator=self.gen)

    def reset(self):
        return self.obs, self.priv

    def get_observations(self):
        return self.obs

    def get_privileged_observations(self):
        return self.priv

    def step(self, actions):
        self.actions.append(actions)
        self._draw()
        return self.obs, self.priv, torch.zeros(N), torch.zeros(N, dtype=torch.bool), {}


def teacher_cfg():
    from legged_gym_amd.envs.go1.go1_config import Go1RoughTeacherCfgPPO
    from legged_gym_amd.utils.helpers import class_to_dict
    cfg = class_to_dict(Go1RoughTeacherCfgPPO())
    cfg["runner"]["num_steps_per_env"] = T
    cfg["policy"].update(actor_hidden_dims=[32], critic_hidden_dims=[16])
    cfg["algorithm"].update(num_mini_batches=2, num_learning_epochs=1)
    return cfg


def distill_cfg():
    from legged_gym_amd.envs.go1.go1_config import Go1RoughDistillCfgPPO
    from legged_gym_amd.utils.helpers import class_to_dict
    cfg = class_to_dict(Go1RoughDistillCfgPPO())
    cfg["runner"]["num_steps_per_env"] = T
    cfg["policy"].update(student_hidden_dims=HID, teacher_hidden_dims=[32])
    cfg["algorithm"]["gradient_length"] = G
    return cfg


def test_configs_and_registry():
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfgPPO
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.envs.go1.go1_config import (Go1RoughAsymHistCfg, Go1RoughDistillCfgPPO,
                                                    Go1RoughTeacherCfgPPO)
    from legged_gym_amd.utils.helpers import class_to_dict
    from legged_gym_amd.utils.task_registry import task_registry
    assert not hasattr(LeggedRobotCfgPPO.runner, "privileged_actor")      # only the new config has the key
    env_cfg, train_cfg = task_registry.get_cfgs("go1_rough_teacher")
    assert isinstance(train_cfg, Go1RoughTeacherCfgPPO) and train_cfg.runner.privileged_actor is True
    assert env_cfg is task_registry.get_cfgs("go1_rough_asym")[0] and env_cfg.env.num_privileged_obs == 253
    assert task_registry.get_task_class("go1_rough_teacher") is Go1
    env_cfg, train_cfg = task_registry.get_cfgs("go1_rough_distill")
    assert isinstance(env_cfg, Go1RoughAsymHistCfg) and isinstance(train_cfg, Go1RoughDistillCfgPPO)
    assert task_registry.get_task_class("go1_rough_distill") is Go1
    assert env_cfg.env.num_privileged_obs == 253 and env_cfg.history.frames == 5
    d = class_to_dict(train_cfg)
    assert d["runner"]["policy_class_name"] == "StudentTeacher" and d["runner"]["algorithm_class_name"] == "Distillation"
    assert d["runner"]["num_steps_per_env"] == 24
    assert d["policy"] == dict(activation="elu", init_noise_std=0.1, student_hidden_dims=[512, 256, 128],
                               teacher_hidden_dims=[512, 256, 128])
    assert d["algorithm"] == dict(gradient_length=12, learning_rate=1e-3, loss_type="mse", max_grad_norm=None,
                                  num_learning_epochs=1)
    # a teacher's run and the student's share a log root: --load_run finds the teacher
    assert d["runner"]["experiment_name"] == class_to_dict(Go1RoughTeacherCfgPPO())["runner"]["experiment_name"]


def test_privileged_actor_runner_trains_on_the_privileged_row():
    from legged_gym_amd.rl.runner import OnPolicyRunner
    env = StandInEnv()
    torch.manual_seed(0)
    runner = OnPolicyRunner(env, teacher_cfg(), None, device="cpu")
    ac = runner.alg.actor_critic
    assert ac.actor[0].in_features == P and ac.critic[0].in_features == P
    st = runner.alg.storage
    assert st.observations.shape == (T, N, P) and st.privileged_observations is None   # the row is held once
    seen = []
    orig = runner.alg.act
    runner.alg.act = lambda obs, cobs: (seen.append((obs, cobs)), orig(obs, cobs))[1]
    first = env.priv
    runner.learn(1)
    assert len(seen) == T and all(o is c and o.shape == (N, P) for o, c in seen)
    assert seen[0][0] is first
    assert set(runner.last_iteration_stats) >= {"value_loss", "surrogate_loss", "learning_rate"}
    policy = runner.get_inference_policy()
    with torch.inference_mode():
        assert torch.equal(policy(env.priv), ac.actor(env.priv))
    # refusals
    with pytest.raises(ValueError, match="privileged row"):
        OnPolicyRunner(StandInEnv(num_privileged_obs=None), teacher_cfg(), None, device="cpu")
    cfg = teacher_cfg()
    cfg["algorithm"]["symmetry"] = {"use_data_augmentation": True}
    with pytest.raises(ValueError, match="algorithm.symmetry"):
        OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    cfg = teacher_cfg()
    cfg["runner"]["empirical_normalization"] = True
    with pytest.raises(ValueError, match="empirical_normalization"):
        OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    # the flag absent or off: the actor reads the observations, the critic the privileged row, as before
    cfg = teacher_cfg()
    del cfg["runner"]["privileged_actor"]
    plain = OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    assert plain.alg.actor_critic.actor[0].in_features == W and plain.alg.actor_critic.critic[0].in_features == P
    assert plain.alg.storage.privileged_observations.shape == (T, N, P)


def test_distillation_runner_end_to_end_on_cpu(tmp_path, capsys):
    from legged_gym_amd.rl.runner import OnPolicyRunner
    torch.manual_seed(0)
    teacher = OnPolicyRunner(StandInEnv(), teacher_cfg(), None, device="cpu")
    teacher.learn(1)
    ckpt = str(tmp_path / "teacher.pt")
    teacher.save(ckpt)
    env = StandInEnv(seed=1)
    runner = OnPolicyRunner(env, distill_cfg(), str(tmp_path / "run"), device="cpu")
    os.makedirs(runner.log_dir, exist_ok=True)
    assert isinstance(runner.alg, Distillation) and isinstance(runner.alg.actor_critic, StudentTeacher)
    with pytest.raises(ValueError, match="no teacher"):
        runner.learn(1)
    runner.load(ckpt)
    assert runner.current_learning_iteration == 0                       # a teacher-only load: not a resumed run
    for k, v in teacher.alg.actor_critic.actor.state_dict().items():
        assert torch.equal(runner.alg.policy.teacher.state_dict()[k], v), k
    runner.learn(3)
    out = capsys.readouterr().out
    assert "Behavior loss:" in out and "Surrogate loss:" not in out and "Value function loss:" not in out
    loss = runner.last_iteration_stats["behavior_loss"]
    assert np.isfinite(loss) and loss > 0 and "value_loss" not in runner.last_iteration_stats
    assert len(env.actions) == 3 * T
    policy = runner.get_inference_policy()
    with torch.inference_mode():
        assert torch.equal(policy(env.obs), runner.alg.policy.student(env.obs))
    # save / resume restores the student, the optimizer and iter
    path = os.path.join(runner.log_dir, "model_3.pt")
    assert os.path.exists(path)
    again = OnPolicyRunner(StandInEnv(seed=2), distill_cfg(), None, device="cpu")
    again.load(path)
    assert again.current_learning_iteration == 3 and again.alg.policy.loaded_teacher
    for k, v in runner.alg.policy.state_dict().items():
        assert torch.equal(again.alg.policy.state_dict()[k], v), k
    a, b = runner.alg.optimizer.state_dict()["state"], again.alg.optimizer.state_dict()["state"]
    assert a.keys() == b.keys() and len(a) > 0
    for i in a:
        assert torch.equal(a[i]["exp_avg"], b[i]["exp_avg"]) and torch.equal(a[i]["exp_avg_sq"], b[i]["exp_avg_sq"])
    # refusals of the runner
    cfg = distill_cfg()
    cfg["runner"]["empirical_normalization"] = True
    with pytest.raises(ValueError, match="empirical_normalization"):
        OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    with pytest.raises(ValueError, match="privileged row"):
        OnPolicyRunner(StandInEnv(num_privileged_obs=None), distill_cfg(), None, device="cpu")
    cfg = distill_cfg()
    cfg["runner"]["num_steps_per_env"] = 3
    with pytest.raises(ValueError, match="gradient_length"):
        OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    cfg = distill_cfg()
    cfg["algorithm"]["loss_type"] = "huber"
    with pytest.raises(ValueError, match="loss_type"):
        OnPolicyRunner(StandInEnv(), cfg, None, device="cpu")
    # a teacher checkpoint that carries normaliser statistics
    d = torch.load(ckpt, weights_only=True)
    d["obs_norm_state_dict"] = {}
    torch.save(d, ckpt)
    with pytest.raises(ValueError, match="normaliser"):
        OnPolicyRunner(StandInEnv(), distill_cfg(), None, device="cpu").load(ckpt)
