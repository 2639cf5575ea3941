"""GPU: teacher-student distillation on the fused update (rsl_rl 2.x Distillation):
lgx_bc_loss_bwd on its own against the float64 statement of tests/distillation_ref.py, the fused chunk
gradient and the whole update against the autograd path, the one-launch rollout, go1_rough_teacher ->
go1_rough_distill end to end, and off meaning off for PPO.

Tolerances are those of tests/test_gpu_symmetry.py and tests/test_gpu_mirror_loss.py: gradient
|d| <= 1e-5 + 2e-3 |g|, losses 1e-4 relative, and the full-update criterion of tests/test_gpu_ppo.py (at
most 1e-3 of the parameters off by more than 1e-5).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import distillation_ref as ref64
from legged_gym_amd.rl.distillation import Distillation
from legged_gym_amd.rl.student_teacher import StudentTeacher
from legged_gym_amd.sim import abi
from legged_gym_amd.utils.task_registry import task_registry
from oracle_backend import make_env
from test_gpu_ppo import _CallCounter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACT, PRIV = 12, 253
EINVAL = -1
CANARY = 64


def close(a, b, what):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    err = (a - b).abs()
    assert (err <= 1e-5 + 2e-3 * b.abs()).all(), (what, err.max().item(), b.abs().max().item())


def loss_close(a, b, what):
    assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (what, a, b)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def lgx():
    from legged_gym_amd.sim import lib as lgxlib
    return lgxlib.load()


def vp(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- the launch alone
class Launch:
    """Inputs and output buffers of one lgx_bc_loss_bwd call over M rows, with a canary block behind
    every buffer and EXTRA rows of head_in past M that the launch must leave alone."""
    EXTRA = 3

    def __init__(self, M, H, A, seed=0):
        self.lib, self.M, self.H, self.A = lgx(), M, H, A
        g = torch.Generator(device=DEV).manual_seed(seed + M + H)
        r = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.Y3 = torch.nn.functional.elu(r(M + self.EXTRA, H))        # post-ELU activations
        self.W4, self.b4, self.target = r(A, H) * 0.1, r(A) * 0.1, r(M, A)
        self.scale = 1.0 / (8 * A)
        lay = (C.c_int64 * 3)()
        assert self.lib.lgx_bc_loss_bwd_layout(M, A, H, lay) == 0
        self.wgs = -(-M // 32)
        assert tuple(lay)[:2] == (self.wgs, self.wgs * (A * H + A + H)) and lay[2] <= 96 * 1024
        self.sizes = dict(head_in=(M + self.EXTRA) * H, loss_parts=int(lay[0]), head_parts=int(lay[1]))
        self.reset()

    def reset(self):
        self.buf = {k: torch.full((n + CANARY,), 777.0, device=DEV) for k, n in self.sizes.items()}
        self.buf["head_in"][:self.sizes["head_in"]].copy_(self.Y3.reshape(-1))

    def call(self, **over):
        a = dict(head_in=vp(self.buf["head_in"]), W4=vp(self.W4), b4=vp(self.b4), target=vp(self.target), rows=self.M,
                 A=self.A, H=self.H, scale=self.scale, loss_parts=vp(self.buf["loss_parts"]),
                 head_parts=vp(self.buf["head_parts"]))
        a.update(over)
        return self.lib.lgx_bc_loss_bwd(a["head_in"], a["W4"], a["b4"], a["target"], a["rows"], a["A"], a["H"],
                                        a["scale"], a["loss_parts"], a["head_parts"], None)

    def results(self):
        torch.cuda.synchronize()
        M, H, A = self.M, self.H, self.A
        for k, n in self.sizes.items():
            assert torch.all(self.buf[k][n:] == 777.0), f"{k}: canary overwritten"
        head = self.buf["head_in"][:self.sizes["head_in"]].view(M + self.EXTRA, H)
        hp = self.buf["head_parts"][:self.sizes["head_parts"]].view(self.wgs, A * H + A + H)
        return dict(dz3=head[:M].clone(), past=head[M:].clone(), dW4=hp[:, :A * H].double().sum(0).view(A, H),
                    db4=hp[:, A * H:A * H + A].double().sum(0), db3=hp[:, A * H + A:].double().sum(0),
                    sumsq=float(self.buf["loss_parts"][:self.wgs].double().sum()),
                    raw=[bits(self.buf[k]) for k in self.sizes])


@pytest.mark.parametrize("M,H,A", [(5, 128, 12), (37, 128, 12), (64, 128, 12), (37, 64, 16)])
def test_launch_matches_the_float64_statement(gpu, M, H, A):
    L = Launch(M, H, A)
    assert L.call() == 0
    out = L.results()
    want = ref64.head(L.Y3[:M].cpu().numpy(), L.W4.cpu().numpy(), L.b4.cpu().numpy(), L.target.cpu().numpy(), L.scale)
    for k in ("dz3", "dW4", "db4", "db3"):
        print(f"lgx_bc_loss_bwd M={M} H={H} A={A} {k}: max |d| "
              f"{(out[k].double().cpu() - torch.as_tensor(want[k])).abs().max().item():.3e}")
        close(out[k], want[k], k)
    loss_close(out["sumsq"], want["sumsq"], "sum d^2")
    assert torch.equal(out["past"], L.Y3[M:]), "rows past M were written"     # in place, rows < M only
    L.reset()                                                                  # no atomics: the same bits again
    assert L.call() == 0
    for a, b in zip(out["raw"], L.results()["raw"]):
        assert np.array_equal(a, b)


def test_launch_refuses_bad_arguments(gpu):
    L = Launch(37, 128, 12)
    before = {k: v.clone() for k, v in L.buf.items()}
    lib = L.lib
    bad = [dict(head_in=None), dict(W4=None), dict(b4=None), dict(target=None), dict(loss_parts=None),
           dict(head_parts=None), dict(rows=0), dict(rows=-3), dict(A=0), dict(A=abi.PPO_MAX_ACTIONS + 1),
           dict(H=0), dict(H=120), dict(H=1024), dict(scale=float("nan")), dict(scale=float("inf")),
           dict(head_in=C.c_void_p(L.buf["head_in"].data_ptr() + 4))]
    for over in bad:
        assert L.call(**over) == EINVAL, over
        assert b"lgx_bc_loss_bwd" in lib.lgx_last_error(), over
    torch.cuda.synchronize()
    for k, v in L.buf.items():
        assert torch.equal(v, before[k]), f"{k}: a refused call launched"
    lay = (C.c_int64 * 3)()
    assert lib.lgx_bc_loss_bwd_layout(37, 12, 128, None) == EINVAL
    assert lib.lgx_bc_loss_bwd_layout(37, 12, 1024, lay) == EINVAL and b"LDS" in lib.lgx_last_error()


def test_loss_reduce_is_a_fixed_order_sum(gpu):
    lib = lgx()
    g = torch.Generator(device=DEV).manual_seed(5)
    parts = torch.rand(1000 + CANARY, device=DEV, generator=g)
    outs = []
    for _ in range(2):
        out = torch.full((1 + CANARY,), 777.0, device=DEV)
        assert lib.lgx_bc_loss_reduce(vp(parts), 1000, 0.25, vp(out), None) == 0
        torch.cuda.synchronize()
        assert torch.all(out[1:] == 777.0)
        outs.append(out[:1].clone())
    assert torch.equal(*outs)
    loss_close(float(outs[0]), 0.25 * float(parts[:1000].double().sum()), "reduce")
    for args in ((None, 4, 1.0, vp(parts)), (vp(parts), 4, 1.0, None), (vp(parts), 0, 1.0, vp(parts)),
                 (vp(parts), 4, float("nan"), vp(parts))):
        assert lib.lgx_bc_loss_reduce(*args, None) == EINVAL and b"lgx_bc_loss_reduce" in lib.lgx_last_error()


# ---------------------------------------------------------------- fused against autograd
HID = [512, 256, 128]


def make_pair(W=475, N=64, T=4, G=2, epochs=2, max_grad_norm=None, seed=0):
    """(autograd, fused) Distillation on identical policies and identical stored rollouts (written
    through act(): the rollout's one fused launch)."""
    torch.manual_seed(seed)
    policy = StudentTeacher(W, PRIV, ACT, student_hidden_dims=HID, teacher_hidden_dims=[128, 64]).to(DEV)
    policy.loaded_teacher = True
    pair = []
    for fused in (False, True):
        alg = Distillation(copy.deepcopy(policy), num_learning_epochs=epochs, gradient_length=G, learning_rate=1e-3,
                           max_grad_norm=max_grad_norm, device=DEV, use_fused_update=fused)
        assert (alg._fused is not None) == fused
        alg.init_storage(N, T, [W], [PRIV], [ACT])
        pair.append(alg)
    fill(*pair)
    return pair


def fill(*algs, seed=3):
    alg = algs[0]
    st = alg.storage
    for a in algs:
        a.storage.clear()
    T, N, W = st.observations.shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs, tobs = torch.randn(T, N, W, device=DEV, generator=g), torch.randn(T, N, PRIV, device=DEV, generator=g)
    with torch.inference_mode():
        for t in range(T):
            for a in algs:
                a.act(obs[t], tobs[t])
                a.process_env_step(None, torch.zeros(N, dtype=torch.bool, device=DEV), {})
    return obs, tobs


@pytest.mark.parametrize("W", [475, 235])
def test_fused_chunk_gradient_matches_autograd(gpu, W):
    """M = 2 x 64 = 128 rows; 235: the layer-1 K padding (235 -> 256 columns of the storage rows)."""
    ref, fus = make_pair(W=W)
    assert torch.equal(ref.storage.padded, fus.storage.padded)
    for c in range(2):
        want, got = ref.chunk_gradient(c), fus.chunk_gradient(c)
        assert ref.fused is False and fus.fused is True
        print(f"chunk gradient W={W} chunk {c}: max |d| {(got - want).abs().max().item():.3e}, max |g| "
              f"{want.abs().max().item():.3e}")
        close(got, want, f"W={W} chunk {c}")
    # against float64 as well
    lin = [m for m in ref.policy.student if isinstance(m, torch.nn.Linear)]
    params = [(l.weight.detach().double().cpu().numpy(), l.bias.detach().double().cpu().numpy()) for l in lin]
    st = ref.storage
    _, _, grads = ref64.chunk_loss_grad(params, st.observations[:2].double().cpu().numpy(),
                                        st.privileged_actions[:2].double().cpu().numpy())
    want = np.concatenate([np.concatenate([gw.reshape(-1), gb.reshape(-1)]) for gw, gb in grads])
    close(fus.chunk_gradient(0), want, "float64")


def test_chunk_the_kernels_do_not_take_runs_on_autograd(gpu):
    """M = 2 x 20 = 40 rows is no multiple of 32: the whole update runs on autograd (over the flat
    buffers), never a mix."""
    ref, fus = make_pair(W=235, N=20)
    assert fus._fused is not None
    want, got = ref.chunk_gradient(1), fus.chunk_gradient(1)
    assert fus.fused is False
    close(got, want, "M=40")
    fus._fused.lib = spy = _CallCounter(fus._fused.lib)
    l_ref, l_fus = ref.update(), fus.update()
    assert fus.fused is False and set(spy.calls) == {"lgx_adam_clip_mirror"} and spy.calls["lgx_adam_clip_mirror"] == 4
    loss_close(l_fus, l_ref, "loss")
    count_off(fus, ref)


def count_off(fus, ref):
    big = total = 0
    for a, b in zip(fus.policy.student.parameters(), ref.policy.student.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    print(f"full update: {big} of {total} parameters off by more than 1e-5")
    assert big <= 1e-3 * total, (big, total)


@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["noclip", "clip"])
def test_fused_update_matches_the_autograd_update(gpu, max_grad_norm):
    """T = 4, gradient_length = 2, 2 epochs: four Adam steps, the limb images kept by the Adam mirrors."""
    ref, fus = make_pair(max_grad_norm=max_grad_norm)
    teacher0, std0 = copy.deepcopy(fus.policy.teacher.state_dict()), fus.policy.std.detach().clone()
    student0 = [p.detach().clone() for p in fus.policy.student.parameters()]
    obs = fus.storage.observations[0].clone()
    with torch.no_grad():
        mean0 = fus.policy.act_inference(obs)
    fus._fused.lib = spy = _CallCounter(fus._fused.lib)
    l_ref, l_fus = ref.update(), fus.update()
    assert ref.fused is False and fus.fused is True
    assert spy.calls == {"lgx_bc_loss_bwd_layout": 1, "lgx_split_bf16": 1, "lgx_gemm_nt": 4 * 5, "lgx_bc_loss_bwd": 4, "lgx_gemm_tn": 4 * 3,
                         "lgx_reduce_slices": 4, "lgx_adam_clip_mirror": 4, "lgx_bc_loss_reduce": 1}, spy.calls
    print(f"behaviour loss fused {l_fus:.8f} autograd {l_ref:.8f}")
    loss_close(l_fus, l_ref, "behaviour loss")
    count_off(fus, ref)
    assert all((a - b).abs().max() > 1e-4 for a, b in zip(fus.policy.student.parameters(), student0))
    for k, v in fus.policy.teacher.state_dict().items():                 # teacher and std: bit-identical
        assert torch.equal(v, teacher0[k]), k
    assert torch.equal(fus.policy.std.detach(), std0)
    assert int(fus.optimizer.step_dev.item()) == 4 and fus.storage.step == 0
    # the Adam step's limb mirrors equal a fresh split of the stepped weights
    f = fus._fused
    kept = [b.clone() for b in f.nl + f.nlt[1:]]
    assert f.lib.lgx_split_bf16(f.copy_jobs, len(f.copy_jobs), None) == 0
    torch.cuda.synchronize()
    for a, b in zip(kept, f.nl + f.nlt[1:]):
        assert torch.equal(a, b)
    # the rollout MLP sees the stepped student: act() after the update, then a second update
    with torch.no_grad():
        mean1 = fus.policy.act_inference(obs)                            # (the fused MLP: no-grad, on the GPU)
    assert fus.policy._fused_student.last_x3 is not None
    want = fus.policy.student(obs)
    close(mean1, want, "rollout mean after the update")
    assert (mean1 - mean0).abs().max() > 1e-3
    fill(ref, fus, seed=4)
    lin = list(fus.policy.student.parameters())
    loss, _ = fus._chunk_loss(0)
    want = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, lin)])
    close(fus.chunk_gradient(0), want, "second update's gradient")
    assert fus.fused is True
    l2 = fus.update()
    assert np.isfinite(l2) and int(fus.optimizer.step_dev.item()) == 8


def test_deferred_update_reads_the_same_loss(gpu):
    _, a = make_pair(epochs=1)
    _, b = make_pair(epochs=1)
    want = a.update()
    assert b.update(defer=True) is None
    assert b.resolve() == want and b.resolve() is None
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)


# ---------------------------------------------------------------- the rollout
def forward_bound(net, x):
    """(float64 forward of an nn.Sequential MLP, a bound on the f32 kernels' error): per layer the
    split-bf16 products' K 2^-24 sum |a b| of tests/test_gpu_split_products.py (with the bias as one more term),
    the error coming in carried through |W|, and 2^-22 for the ELU's v_exp_f32 (1-Lipschitz otherwise)."""
    x = x.double()
    err = torch.zeros_like(x)
    for m in net:
        if isinstance(m, torch.nn.Linear):
            Wd, b = m.weight.detach().double(), m.bias.detach().double()
            err = err @ Wd.abs().T + (m.in_features + 1) * 2.0 ** -24 * (x.abs() @ Wd.abs().T + b.abs())
            x = x @ Wd.T + b
        else:
            x = torch.nn.functional.elu(x)
            err = err + 2.0 ** -22
    return x, err


def test_rollout_rows(gpu):
    ref, fus = make_pair(W=475, N=64)
    obs, tobs = fill(fus, seed=9)
    st = fus.storage
    assert fus.policy._fused_teacher.last_x3 is not None                  # the fused launch ran
    want, bound = forward_bound(fus.policy.teacher, tobs.view(-1, PRIV))
    err = (st.privileged_actions.view(-1, ACT).double() - want).abs()
    print(f"privileged_actions: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(bits(st.observations), bits(obs))               # bit for bit
    assert st.padded.shape[-1] == 512 and torch.all(st.padded[..., 475:] == 0)
    st.clear()
    with torch.inference_mode():
        torch.manual_seed(1)
        a = fus.act(obs[0], tobs[0])
        torch.manual_seed(1)
        mean = fus.policy.act_inference(obs[0])
        b = torch.normal(mean, fus.policy.std.expand_as(mean))            # one [N, A] draw, as Normal.sample
    assert torch.equal(a, b)


# ---------------------------------------------------------------- end to end
def test_teacher_then_distill_end_to_end(gpu, tmp_path):
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    env = make_env("go1_rough_teacher", num_envs=64, device=DEV, backend="lgx")
    cfg = class_to_dict(task_registry.get_cfgs("go1_rough_teacher")[1])
    assert cfg["runner"]["privileged_actor"] is True
    torch.manual_seed(0)
    (tmp_path / "teacher").mkdir()
    (tmp_path / "student").mkdir()
    teacher = OnPolicyRunner(env, cfg, str(tmp_path / "teacher"), device=DEV)
    assert teacher.alg.actor_critic.actor[0].in_features == PRIV and teacher.alg.storage.privileged_observations is None
    teacher.learn(2, init_at_random_ep_len=True)
    ckpt = tmp_path / "teacher" / "model_2.pt"
    assert ckpt.exists()
    env = make_env("go1_rough_distill", num_envs=64, device=DEV, backend="lgx")
    assert (env.num_obs, env.num_privileged_obs) == (475, PRIV)
    cfg = class_to_dict(task_registry.get_cfgs("go1_rough_distill")[1])
    runner = OnPolicyRunner(env, cfg, str(tmp_path / "student"), device=DEV)
    policy = runner.alg.policy
    student0 = [p.detach().clone() for p in policy.student.parameters()]
    runner.load(str(ckpt))
    assert runner.current_learning_iteration == 0 and policy.loaded_teacher
    for k, v in torch.load(ckpt, weights_only=True)["model_state_dict"].items():
        if k.startswith("actor."):
            assert torch.equal(policy.teacher.state_dict()[k[len("actor."):]].cpu(), v.cpu()), k
    assert all(torch.equal(a, b) for a, b in zip(policy.student.parameters(), student0))
    runner.learn(3, init_at_random_ep_len=True)
    assert runner.alg.fused is True                                       # 12 x 64 = 768 rows per chunk
    loss = runner.last_iteration_stats["behavior_loss"]
    assert np.isfinite(loss) and loss > 0 and "value_loss" not in runner.last_iteration_stats
    path = tmp_path / "student" / "model_3.pt"
    assert path.exists()
    other = OnPolicyRunner(env, cfg, None, device=DEV)
    other.load(str(path))
    assert other.current_learning_iteration == 3 and other.alg.policy.loaded_teacher
    for (k, a), b in zip(policy.state_dict().items(), other.alg.policy.state_dict().values()):
        assert torch.equal(a, b), k
    o, p = runner.alg.optimizer, other.alg.optimizer
    assert torch.equal(o.m, p.m) and torch.equal(o.v, p.v) and int(p.step_dev.item()) == 3 * 2
    act = runner.get_inference_policy(device=DEV)
    with torch.inference_mode():
        obs = env.get_observations()
        close(act(obs), policy.student(obs), "inference policy")


# ---------------------------------------------------------------- off is off
def test_ppo_update_does_not_touch_the_new_code(gpu):
    """Two fresh go1_rough-shaped fused PPO updates give the same bits, and none of the library calls
    they make is one of this feature's."""
    from test_gpu_ppo import make_pair as ppo_pair
    params = []
    for _ in range(2):
        _, fus = ppo_pair(N=256)
        fus._fused.lib = spy = _CallCounter(fus._fused.lib)
        torch.manual_seed(11)
        fus.update()
        assert not any(name.startswith("lgx_bc_") for name in spy.calls), spy.calls
        params.append([bits(p) for p in fus.actor_critic.parameters()])
    for a, b in zip(*params):
        assert np.array_equal(a, b)
