"""GPU: the fused PPO update (lgx PPO kernels + hand-written GEMMs over flat buffers) against the
autograd formulation of rsl_rl v1.0.x PPO.update (legged_gym_amd/rl/ppo.py, pinned on CPU by
tests/test_ppo.py) and against oracle/ppo_oracle.py (numpy float64, hand-derived gradients).

Tolerances (float32; different reduction orders): minibatch gradient |d| <= 1e-5 + 2e-3 |g|;
after a full update (2 epochs x 4 minibatches of Adam) identical learning-rate sequence, losses
to 1e-4 relative, parameters to 2 Adam steps of the smallest learning rate for the few
coordinates whose gradient is at rounding level (Adam normalises their sign), 1e-5 otherwise.
"""
import copy
import os

import pytest
import torch

from legged_gym_amd.rl.actor_critic import ActorCritic
from legged_gym_amd.rl.ppo import PPO

pytestmark = pytest.mark.gpu

T, N, OBS, ACT = 6, 1024, 235, 12


def make_pair(schedule="adaptive", cobs=None, hidden=(512, 256, 128), T=T, N=N, epochs=2, obs=OBS):
    """Reference (autograd) and fused PPO on identical storage; cobs = privileged critic
    observation width (None: the critic reads the actor's observations); T x N transitions in
    4 minibatches, `epochs` learning epochs."""
    torch.manual_seed(0)
    ac = ActorCritic(obs, cobs or obs, ACT, list(hidden), list(hidden))
    ac2 = copy.deepcopy(ac)
    kw = dict(num_learning_epochs=epochs, num_mini_batches=4, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
              entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0, schedule=schedule, desired_kl=0.01,
              device="cuda:0")
    ref = PPO(ac, use_fused_update=False, **kw)
    fus = PPO(ac2, use_fused_update=True, **kw)
    assert fus._fused is not None and ref._fused is None
    for p in (ref, fus):
        p.init_storage(N, T, [obs], [cobs], [ACT])
    g = torch.Generator(device="cuda:0").manual_seed(3)
    st = ref.storage
    st.observations.copy_(torch.randn(T, N, obs, device="cuda:0", generator=g))
    st.actions.copy_(torch.randn(T, N, ACT, device="cuda:0", generator=g))
    st.rewards.copy_(torch.randn(T, N, 1, device="cuda:0", generator=g))
    st.dones.copy_((torch.rand(T, N, 1, device="cuda:0", generator=g) < 0.1).byte())
    st.values.copy_(torch.randn(T, N, 1, device="cuda:0", generator=g))
    st.actions_log_prob.copy_(torch.randn(T, N, 1, device="cuda:0", generator=g) * 0.3 - 17)
    st.mu.copy_(torch.randn(T, N, ACT, device="cuda:0", generator=g) * 0.1)
    st.sigma.copy_(torch.rand(T, N, ACT, device="cuda:0", generator=g) * 0.5 + 0.75)
    if cobs:
        st.privileged_observations.copy_(torch.randn(T, N, cobs, device="cuda:0", generator=g))
        fus.storage.privileged_observations.copy_(st.privileged_observations)
    st.step = T
    for name in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob", "mu", "sigma"):
        getattr(fus.storage, name).copy_(getattr(st, name))
    fus.storage.step = T
    last = torch.randn(N, 1, device="cuda:0", generator=g)
    for p in (ref, fus):
        p.storage.compute_returns(last, 0.99, 0.95)
    return ref, fus


def autograd_grads(ref, idx):
    st = ref.storage
    B = st.num_transitions_per_env * st.num_envs
    ac = ref.actor_critic
    obs = st.observations.view(B, -1)[idx]
    cobs = st.privileged_observations.view(B, -1)[idx] if st.privileged_observations is not None else obs
    ac.act(obs)
    logp = ac.get_actions_log_prob(st.actions.view(B, -1)[idx])
    value = ac.evaluate(cobs)
    ent = ac.entropy
    ratio = torch.exp(logp - st.actions_log_prob.view(B)[idx])
    adv = st.advantages.view(B)[idx]
    s = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    tv, ret = st.values.view(B, 1)[idx], st.returns.view(B, 1)[idx]
    vc = tv + (value - tv).clamp(-0.2, 0.2)
    vl = torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
    loss = s + vl - 0.01 * ent.mean()
    for p in ac.parameters():
        p.grad = None
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in ac.named_parameters()}


def test_fused_minibatch_gradient_matches_autograd(gpu):
    ref, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    assert fus._fused.loss_bwd      # loss + output-layer backward in one launch (lgx_ppo_loss_bwd)
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        tol = 1e-5 + 2e-3 * b.abs()
        assert ((a - b).abs() <= tol).all(), (n, (a - b).abs().max().item(), b.abs().max().item())


@pytest.mark.parametrize("rows", [1000, 37])
def test_fused_minibatch_gradient_ragged_rows(gpu, rows):
    """Minibatches whose row count is not a multiple of the 32-row loss / head-backward chunk."""
    ref, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0")[:rows]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), (rows, n, (a - b).abs().max().item())


def test_fused_update_single_stream(gpu, monkeypatch):
    """Every backward launch on one stream (LGX_PPO_DW_SIDE=0; default: the weight-gradient GEMMs
    on a second stream next to the dA GEMMs): a full update against autograd."""
    monkeypatch.setenv("LGX_PPO_DW_SIDE", "0")
    ref, fus = make_pair()
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    vl_f, sl_f = fus.update()
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6
    assert getattr(fus._fused, "_side", None) is None


class _CallCounter:
    """Forwards every attribute to the product library and counts the calls per entry point (in the
    style of ppo_trace._LibSpy)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_run_switches_are_read_per_update_call(gpu, monkeypatch):
    """A run switch (LGX_PPO_DW_SIDE as the side stream's on / off) toggled between update() calls
    of ONE object takes effect at the next call (tools/kbench.py update_env relies on it): no
    cross-stream wait with the switch at 0, some with it unset, none again at 0."""
    monkeypatch.delenv("LGX_PPO_DEV_EVENTS", raising=False)   # (device events: joins go through the library)
    _, fus = make_pair()
    f = fus._fused
    f.lib = spy = _CallCounter(f.lib)
    waits = []
    for val in ("0", None, "0"):
        if val is None:
            monkeypatch.delenv("LGX_PPO_DW_SIDE", raising=False)
        else:
            monkeypatch.setenv("LGX_PPO_DW_SIDE", val)
        spy.calls.clear()
        torch.manual_seed(11)
        losses = fus.update()
        assert all(torch.isfinite(torch.tensor(losses)))
        assert spy.calls.get("lgx_adam_clip_mirror_sq", 0) == 8     # 2 epochs x 4 minibatches went through the proxy
        waits.append(spy.calls.get("lgx_stream_wait_event", 0))
    torch.cuda.synchronize()
    assert waits[0] == 0 and waits[1] > 0 and waits[2] == 0, waits


def test_reduce_slices_sum_of_squares(gpu):
    """lgx_reduce_slices_sq: the slice sums as lgx_reduce_slices, and per workgroup the sum of squares
    of what it wrote (float4 and scalar jobs), which together give the gradient's squared norm."""
    import ctypes as C
    from legged_gym_amd.sim import abi
    from legged_gym_amd.sim import lib as lgxlib
    lib = lgxlib.load()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    S, n1, n2 = 16, 4096 + 256, 1001
    src1 = torch.randn(S, n1, device="cuda:0", generator=g)
    src2 = torch.randn(S, n2, device="cuda:0", generator=g)
    dst = torch.zeros(n1 + n2 + 4, device="cuda:0")
    jobs = (abi.LgxReduceJob * 2)()
    for j, (src, off, n) in enumerate(((src1, 0, n1), (src2, n1 + 4, n2))):
        jobs[j].src, jobs[j].dst = src.data_ptr(), dst.data_ptr() + 4 * off
        jobs[j].n, jobs[j].count, jobs[j].job_stride, jobs[j].slices = n, 1, 0, S
        jobs[j].slice_stride, jobs[j].dst_stride = n, 0
    nb = int(lib.lgx_reduce_slices_blocks(jobs, 2, 0))
    assert nb > 2
    sq = torch.full((nb + 1,), -1.0, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lgxlib.check(lib.lgx_reduce_slices_sq(jobs, 2, None, C.c_void_p(sq.data_ptr()), None, stream), "reduce_sq")
    torch.cuda.synchronize()
    ref1, ref2 = src1.sum(0), src2.sum(0)
    assert torch.allclose(dst[:n1], ref1, atol=1e-5) and torch.allclose(dst[n1 + 4:], ref2, atol=1e-5)
    assert (sq[:nb] >= 0).all() and sq[nb].item() == -1.0   # every workgroup wrote its entry, no more
    want = float((dst.double() ** 2).sum())
    assert abs(float(sq[:nb].double().sum()) - want) <= 1e-5 * want
    assert lib.lgx_reduce_slices_sq(jobs, 2, None, None, None, stream) != 0   # (null output refused)


@pytest.mark.parametrize("var,val", [("LGX_PPO_TN_COLSUM", "0"), ("LGX_PPO_DEV_EVENTS", "0"),
                                     ("LGX_PPO_FUSED_SQ", "0")])
def test_fused_update_ab_variants(gpu, monkeypatch, var, val):
    """The update's variants against autograd: the hidden-layer bias gradients from the dA GEMMs'
    ELU' + column-sum epilogue instead of lgx_gemm_tn's column sums (LGX_PPO_TN_COLSUM=0), torch
    events for the cross-stream joins (LGX_PPO_DEV_EVENTS=0), and the clip norm from its own
    sum-of-squares launch instead of the reductions' (LGX_PPO_FUSED_SQ=0)."""
    monkeypatch.setenv(var, val)
    ref, fus = make_pair()
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    vl_f, sl_f = fus.update()
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6
    big = total = 0   # (the criterion of test_fused_update_matches_autograd_update below)
    for (n, a), b in zip(fus.actor_critic.named_parameters(), ref.actor_critic.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    assert big <= 1e-3 * total, (big, total)


def test_bound_join_events_match_recorded_events(gpu, monkeypatch):
    """The backward's cross-stream joins with their device events bound to the producer launches
    (lgx_launch_bind_event, the default) and recorded after them (LGX_PPO_BIND=0): the same kernels
    in the same order, so a full update gives bitwise the same parameters, moments and losses; every
    armed binding was taken by a launch."""
    out = []
    for bind in ("1", "0"):
        monkeypatch.setenv("LGX_PPO_BIND", bind)
        _, fus = make_pair()
        torch.manual_seed(11)
        losses = fus.update()
        torch.cuda.synchronize()
        assert getattr(fus._fused, "_armed", None) is None
        assert fus._fused.lib.lgx_launch_bind_pending() == 0
        o = fus.optimizer
        out.append(([p.detach().clone() for p in fus.actor_critic.parameters()], o.m.clone(), o.v.clone(), losses))
    (pa, ma, va, la), (pb, mb, vb, lb) = out
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert torch.equal(ma, mb) and torch.equal(va, vb) and la == lb


def test_fused_minibatch_gradient_separate_loss_and_head(gpu, monkeypatch):
    """lgx_ppo_loss + lgx_head_bwd_finalize as two launches (LGX_PPO_LOSS_BWD=0) instead of
    lgx_ppo_loss_bwd: minibatch gradient and a full update against autograd."""
    monkeypatch.setenv("LGX_PPO_LOSS_BWD", "0")
    ref, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    assert not fus._fused.loss_bwd
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), n
    ref, fus = make_pair()
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    vl_f, sl_f = fus.update()
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6


@pytest.mark.parametrize("mode", ["auto", "lib", "f32"])
def test_fused_minibatch_gradient_gemm_modes(gpu, monkeypatch, mode):
    """LGX_PPO_GEMM=auto (library GEMM + lgx_bias_act for layers 2..L), =lib (library GEMMs
    with lgx_bias_act / lgx_elu_bwd_colsum everywhere) and the exact-f32 MFMA GEMMs
    (LGX_GEMM_ALGO=f32 instead of the default split-bf16 products) against autograd."""
    if mode == "f32":
        monkeypatch.setenv("LGX_GEMM_ALGO", "f32")
    else:
        monkeypatch.setenv("LGX_PPO_GEMM", mode)
    ref, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    assert fus._fused.lgx_gemm == (mode != "lib")
    assert fus._fused.split == (mode != "f32")
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), (mode, n)


@pytest.mark.parametrize("hidden", [(512, 256, 128, 64), (400, 300), (256, 256, 128, 128, 64, 64, 32)])
def test_fused_other_hidden_stacks(gpu, hidden):
    """Deeper stacks (more reduction jobs / weight mirrors) and widths that are not multiples of
    the GEMM tile (library GEMMs + lgx_elu_bwd_colsum at h/4 = 100, 75): minibatch gradient and
    a full update against autograd."""
    ref, fus = make_pair(hidden=hidden)
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), (hidden, n, (a - b).abs().max().item())
    ref, fus = make_pair(hidden=hidden)
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    vl_f, sl_f = fus.update()
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6


@pytest.mark.parametrize("cobs", [252, OBS])
def test_fused_minibatch_gradient_privileged_critic(gpu, cobs):
    """Privileged critic observations of another width, and of the actor's width (separate rows of
    the same width: the layer-1 weight gradients per network, not the batched shared-input dW1)."""
    ref, fus = make_pair(cobs=cobs)
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), n


def test_fused_minibatch_gradient_library_heads(gpu, monkeypatch):
    """The output layers on library GEMMs (LGX_PPO_HEAD_IN_LOSS=0) instead of inside lgx_ppo_loss."""
    monkeypatch.setenv("LGX_PPO_HEAD_IN_LOSS", "0")
    ref, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
    gref = autograd_grads(ref, idx)
    fus._fused.gradients(idx)
    assert not fus._fused.head_in_loss
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), n


@pytest.mark.parametrize("schedule,cobs,algo", [("adaptive", None, "split"), ("fixed", None, "split"),
                                                ("adaptive", 252, "split"), ("adaptive", None, "f32")])
def test_fused_update_matches_autograd_update(gpu, monkeypatch, schedule, cobs, algo):
    """Full update (one gather of all minibatch rows, Adam-maintained GEMM weight copies); cobs:
    privileged critic observations of another width (two layer-1 inputs and GEMM launches);
    algo: the split-bf16 GEMM products with Adam-maintained limb copies, or exact f32."""
    monkeypatch.setenv("LGX_GEMM_ALGO", algo)
    ref, fus = make_pair(schedule, cobs)
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    vl_f, sl_f = fus.update()
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6
    # end to end after 8 Adam steps the two runs differ only where Adam normalised a rounding-level
    # gradient into a full step of either sign (and what that feeds): a few coordinates.  Every
    # coordinate of every step is checked exactly in test_fused_update_every_step_is_exact.
    big = 0
    total = 0
    for (n, a), b in zip(fus.actor_critic.named_parameters(), ref.actor_critic.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    assert big <= 1e-3 * total, (big, total)


def test_fused_checkpoint_roundtrip(gpu, tmp_path):
    _, fus = make_pair()
    fus.update()
    sd = {"model": fus.actor_critic.state_dict(), "opt": fus.optimizer.state_dict()}
    torch.save(sd, tmp_path / "c.pt")
    d = torch.load(tmp_path / "c.pt", weights_only=True)
    assert set(d["opt"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert int(d["opt"]["state"][0]["step"]) == 8
    _, fus2 = make_pair()
    fus2.actor_critic.load_state_dict(d["model"])
    fus2.optimizer.load_state_dict(d["opt"])
    for a, b in zip(fus.actor_critic.parameters(), fus2.actor_critic.parameters()):
        assert torch.equal(a, b)
    assert torch.equal(fus.optimizer.m, fus2.optimizer.m) and torch.equal(fus.optimizer.v, fus2.optimizer.v)


def test_fused_fixed_schedule_keeps_checkpoint_lr(gpu):
    """schedule='fixed': a restored optimizer lr is the one the next update steps with (as
    torch.optim.Adam's param_groups after load_state_dict), not the config value."""
    ref, fus = make_pair("fixed")
    for p in (ref, fus):
        sd = p.optimizer.state_dict()
        sd["param_groups"][0]["lr"] = 3e-4
        p.optimizer.load_state_dict(sd)
    torch.manual_seed(11)
    ref.update()
    torch.manual_seed(11)
    fus.update()
    assert fus.optimizer.param_groups[0]["lr"] == ref.optimizer.param_groups[0]["lr"] == 3e-4
    assert float(fus._fused.optimizer.lr_dev.item()) == 3e-4
    for a, b in zip(fus.actor_critic.parameters(), ref.actor_critic.parameters()):
        assert (a - b).abs().max().item() <= 2 * 8 * 3e-4


@pytest.mark.parametrize("batched", [False, True])
def test_fused_rollout_act_and_store(gpu, monkeypatch, batched):
    """lgx_ppo_act / lgx_ppo_store == PPO.act + process_env_step + add_transitions (torch).
    Default: the per-step draw of rsl_rl's Normal.sample (torch.normal(mu, std)), same seed ->
    same actions; LGX_BATCHED_NOISE=1: one draw per rollout."""
    from torch.distributions import Normal
    monkeypatch.setenv("LGX_BATCHED_NOISE", "1" if batched else "0")
    _, fus = make_pair()
    st = fus.storage
    st.clear()
    g = torch.Generator(device="cuda:0").manual_seed(7)
    obs = torch.randn(N, OBS, device="cuda:0", generator=g)
    with torch.inference_mode():
        torch.manual_seed(5)
        actions = fus.act(obs, obs).clone()
        assert fus.transition.in_storage
        rew = torch.randn(N, device="cuda:0", generator=g)
        dones = torch.rand(N, device="cuda:0", generator=g) < 0.2
        time_outs = (torch.rand(N, device="cuda:0", generator=g) < 0.5) & dones
        fus.process_env_step(rew, dones, {"time_outs": time_outs})
        assert st.step == 1
        ac = fus.actor_critic
        mean, value = ac.actor(obs), ac.critic(obs)
        torch.manual_seed(5)
        if batched:
            noise = torch.randn((T,) + tuple(mean.shape), device=mean.device)[0]   # one draw per rollout, row 0
            ref_a = mean + ac.std * noise
        else:   # upstream ActorCritic.act: Normal(mean, std).sample()
            ref_a = Normal(mean, mean * 0. + ac.std).sample()
        ref_logp = Normal(mean, ac.std.expand_as(mean)).log_prob(ref_a).sum(-1)
    assert torch.allclose(actions, ref_a, atol=1e-4, rtol=1e-4)
    assert torch.allclose(st.actions[0], actions)
    assert torch.allclose(st.actions_log_prob[0, :, 0], ref_logp, atol=1e-3, rtol=1e-5)
    assert torch.allclose(st.values[0, :, 0], value[:, 0], atol=1e-4, rtol=1e-4)
    assert torch.equal(st.observations[0], obs)
    assert torch.allclose(st.mu[0], mean, atol=1e-4, rtol=1e-4) and torch.equal(st.sigma[0], ac.std.expand_as(mean))
    ref_r = rew + fus.gamma * st.values[0, :, 0] * time_outs.float()
    assert torch.allclose(st.rewards[0, :, 0], ref_r, atol=1e-6, rtol=1e-6)
    assert torch.equal(st.dones[0, :, 0], dones.byte())


@pytest.mark.parametrize("n,cobs", [(1024, None), (1000, None), (1000, 252)])
def test_fused_act_launch_matches_two_launch_form(gpu, monkeypatch, n, cobs):
    """lgx_mlp_x3_forward_act (the rollout MLP with lgx_ppo_act's arithmetic in the actor's last
    layer and the previous step's deferred store in the critic's workgroups) == lgx_mlp_x3_forward +
    lgx_ppo_act(_store), bit for bit: actions, every storage row of three steps (the second and third
    carry the store of the step before), rows not a multiple of the 32-row tile, with and without
    privileged critic observations."""
    names = ("observations", "privileged_observations", "actions", "values", "actions_log_prob", "mu", "sigma",
             "rewards", "dones")
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LGX_FUSED_ACT", fused)
        _, fus = make_pair(cobs=cobs, N=n)
        fus.defer_store = True
        st = fus.storage
        st.clear()
        g = torch.Generator(device="cuda:0").manual_seed(7)
        acts = []
        with torch.inference_mode():
            torch.manual_seed(5)
            for _ in range(3):
                obs = torch.randn(n, OBS, device="cuda:0", generator=g)
                cob = torch.randn(n, cobs, device="cuda:0", generator=g) if cobs else obs
                acts.append(fus.act(obs, cob).clone())
                assert fus.last_act_fused == (fused == "1")
                rew = torch.randn(n, device="cuda:0", generator=g)
                dones = torch.rand(n, device="cuda:0", generator=g) < 0.2
                time_outs = (torch.rand(n, device="cuda:0", generator=g) < 0.5) & dones
                fus.process_env_step(rew, dones, {"time_outs": time_outs})
            fus.flush_store()
        torch.cuda.synchronize()
        outs.append((acts, {k: getattr(st, k)[:3].clone() for k in names if getattr(st, k) is not None}))
    (fa, fs), (ua, us) = outs
    assert all(torch.equal(x, y) for x, y in zip(fa, ua))
    assert fs.keys() == us.keys()
    for k in fs:
        assert torch.equal(fs[k], us[k]), k


def test_fused_act_launch_refused_falls_back(gpu):
    """A network pair the fused act launch refuses (its entry returns an error before launching)
    switches that PPO object to the two-launch form for good, with the same rows."""
    _, a = make_pair(N=1000)
    _, b = make_pair(N=1000)
    lib = b._fused.lib

    class Refusing:   # the library with lgx_mlp_x3_forward_act refusing
        def __getattr__(self, name):
            return (lambda *args: -1) if name == "lgx_mlp_x3_forward_act" else getattr(lib, name)
    b._rollout.lib = Refusing()
    for p in (a, b):
        p.storage.clear()
    g = torch.Generator(device="cuda:0").manual_seed(9)
    obs = torch.randn(1000, OBS, device="cuda:0", generator=g)
    with torch.inference_mode():
        torch.manual_seed(4)
        xa = a.act(obs, obs).clone()
        torch.manual_seed(4)
        xb = b.act(obs, obs).clone()
    torch.cuda.synchronize()
    assert a.last_act_fused and not b.last_act_fused and b._rollout.fused_off
    assert torch.equal(xa, xb)
    for k in ("observations", "actions", "values", "actions_log_prob", "mu", "sigma"):
        assert torch.equal(getattr(a.storage, k)[0], getattr(b.storage, k)[0]), k


def test_fused_minibatch_gradient_matches_numpy_oracle(gpu):
    """The fused minibatch gradient (HIP kernels) against oracle/ppo_oracle.py's hand-derived
    float64 gradient of rsl_rl's PPO loss (independent of torch autograd and of rl/ppo.py):
    |d| <= 1e-5 + 2e-3 |g|, losses to 1e-4."""
    from ppo_oracle_io import oracle_minibatch_grads, grad_deviation
    _, fus = make_pair()
    idx = torch.randperm(T * N, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(8))[: T * N // 4]
    fus._fused.gradients(idx)
    want = oracle_minibatch_grads(fus, idx)
    worst, name = grad_deviation(fus.actor_critic, want[3], rtol=2e-3)
    assert worst <= 1.0, (worst, name)


@pytest.mark.parametrize("hidden", [(512, 256, 128), (384, 128, 128, 256)])
def test_adam_limb_mirrors_equal_a_fresh_split(gpu, hidden):
    """The GEMM weight copies the Adam step writes (split-bf16 limb images of W_1 .. W_L and of
    W_k^T, lgx_adam_clip_mirror*) equal a fresh lgx_split_bf16 of the updated parameters, bit for
    bit."""
    import ctypes as C
    ref, fus = make_pair(hidden=hidden, epochs=1)
    fus.update()
    f = fus._fused
    torch.cuda.synchronize()
    nl, nlt = f.limb_bufs
    bufs = [b for grp in nl if grp is not None for b in (grp if isinstance(grp, tuple) else (grp,))]
    bufs += [b for b in nlt if b is not None]
    assert bufs
    kept = [b.clone() for b in bufs]
    for b in bufs:
        b.fill_(-1)
    f.check(f.lib.lgx_split_bf16(f.copy_jobs, len(f.copy_jobs), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "split_bf16")
    torch.cuda.synchronize()
    for a, b in zip(kept, bufs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("schedule", ["adaptive", "fixed"])
def test_fused_update_matches_numpy_oracle(gpu, schedule):
    """A full fused update (2 epochs x 4 minibatches, Adam, adaptive or fixed learning rate)
    against the oracle's float64 update from the same parameters, storage and permutation:
    same learning-rate sequence, losses to 1e-4, parameters within the rule of the
    fused-vs-autograd test."""
    from ppo_oracle_io import oracle_update, param_deviation
    _, fus = make_pair(schedule)
    want = oracle_update(fus, seed=13)
    torch.manual_seed(13)
    vl, sl = fus.update()
    assert fus.learning_rate == pytest.approx(want[3], rel=1e-9)
    assert abs(vl - want[4]) <= 1e-4 * abs(want[4]) + 1e-6 and abs(sl - want[5]) <= 1e-4 * abs(want[5]) + 1e-6
    dmax, big, total = param_deviation(fus.actor_critic, want)
    assert big <= 1e-3 * total, (big, total, dmax)


@pytest.mark.parametrize("schedule,cobs,algo", [("adaptive", None, "split"), ("fixed", None, "split"),
                                                ("adaptive", 252, "split"), ("adaptive", None, "f32")])
def test_fused_update_every_step_is_exact(gpu, monkeypatch, schedule, cobs, algo):
    """Every coordinate of every optimizer step of a full fused update (2 epochs x 4 minibatches),
    recorded as it runs (tests/ppo_trace.py):
      * the flat gradient the step consumed == the autograd gradient (rl/ppo.py's loss, pinned
        against the numpy oracle on CPU) at the SAME parameters and rows: |d| <= 1e-5 + 2e-3 |g|,
        so the GEMM weight mirrors the previous Adam step wrote (limb images) are checked too;
      * the parameters / moments after the step == float64 clip_grad_norm_ + torch Adam applied
        to that gradient from the recorded state: |d| <= 1e-6 + 1e-3 lr (p), 1e-5 relative (m, v:
        the f32 global norm);
      * the learning rate the step used == the adaptive schedule's (same sequence as autograd)."""
    from ppo_trace import StepTrace, adam64, flat_view
    monkeypatch.setenv("LGX_GEMM_ALGO", algo)
    ref, fus = make_pair(schedule, cobs)
    tr = StepTrace(fus._fused)
    torch.manual_seed(11)
    fus.update()
    tr.close()
    torch.manual_seed(11)
    ref.update()
    assert fus.learning_rate == ref.learning_rate
    assert len(tr.steps) == 8
    params = list(ref.actor_critic.parameters())
    for t, rec in enumerate(tr.steps):
        with torch.no_grad():      # the reference network at the recorded parameters
            for p, q in zip(params, fus._fused.optimizer.params):
                off = fus._fused.off[id(q)]
                p.copy_(rec["p0"][off:off + q.numel()].view_as(p))
        g_ref = flat_view(fus._fused, list(autograd_grads(ref, rec["idx"]).values()))
        g = rec["g"].double()
        bad = ((g - g_ref).abs() > 1e-5 + 2e-3 * g_ref.abs()).sum().item()
        assert bad == 0, (t, bad, (g - g_ref).abs().max().item())
        p_want, m_want, v_want = adam64(rec, fus.max_grad_norm)
        dp = (rec["p1"].double() - p_want).abs()
        assert (dp <= 1e-6 + 1e-3 * rec["lr"]).all(), (t, dp.max().item(), rec["lr"])
        # m = b1 m0 + (1 - b1) g may cancel: relative to the magnitudes of its two terms
        m_scale = 0.9 * rec["m0"].double().abs() + (m_want - 0.9 * rec["m0"].double()).abs()
        assert ((rec["m1"].double() - m_want).abs() <= 1e-5 * m_scale + 1e-12).all(), t
        assert ((rec["v1"].double() - v_want).abs() <= 2e-5 * v_want.abs() + 1e-18).all(), t
        if t > 0:   # every step starts from the previous step's result
            assert torch.equal(rec["p0"], tr.steps[t - 1]["p1"])


@pytest.mark.parametrize("obs,cobs", [(48, None), (169, None), (48, 187)])
def test_fused_update_narrow_inputs_every_step_is_exact(gpu, obs, cobs):
    """Input widths whose padded layer-1 rows are narrower than lgx_gemm_tn's 128-column tiles
    (Go1 flat 48, Cassie 169; a privileged critic of 187): dW1 then runs on the library bmm and db_1
    comes from the dA_1 GEMM's column-sum epilogue on the main stream, after the side stream's last
    join.  Its reduction goes with dW1's on the main stream (in the side stream's early
    reduction it read the partials before dA_1 wrote them).  The default two-stream schedule, every
    coordinate of every step as test_fused_update_every_step_is_exact."""
    from ppo_trace import StepTrace, adam64, flat_view
    for var in ("LGX_PPO_DW_SIDE", "LGX_PPO_EARLY_REDUCE", "LGX_PPO_SPLITS"):
        assert var not in os.environ, var
    ref, fus = make_pair("adaptive", cobs, T=24, N=1024, epochs=1, obs=obs)
    f = fus._fused
    tr = StepTrace(f)
    torch.manual_seed(11)
    fus.update()
    tr.close()
    assert 0 not in f.gemm_dw and 0 not in f.colsum and getattr(f, "_side", None) is not None
    assert f.bo[0] in [j.dst // 4 - f.flat_g.data_ptr() // 4 for j in f.jobs_dw1]   # db_1 with dW1, main stream
    torch.manual_seed(11)
    ref.update()
    assert fus.learning_rate == ref.learning_rate
    params = list(ref.actor_critic.parameters())
    for t, rec in enumerate(tr.steps):
        with torch.no_grad():
            for p, q in zip(params, f.optimizer.params):
                off = f.off[id(q)]
                p.copy_(rec["p0"][off:off + q.numel()].view_as(p))
        g_ref = flat_view(f, list(autograd_grads(ref, rec["idx"]).values()))
        g = rec["g"].double()
        bad = ((g - g_ref).abs() > 1e-5 + 2e-3 * g_ref.abs()).sum().item()
        assert bad == 0, (obs, t, bad, (g - g_ref).abs().max().item())
        p_want, _, _ = adam64(rec, fus.max_grad_norm)
        dp = (rec["p1"].double() - p_want).abs()
        assert (dp <= 1e-6 + 1e-3 * rec["lr"]).all(), (obs, t, dp.max().item())


@pytest.mark.parametrize("n_envs", [4096, 8192])
def test_fused_update_bench_shape_every_step_is_exact(gpu, n_envs):
    """The composed update at the shapes bench.py runs: 24 steps x 4096 envs
    (C3: 24,576-row minibatches) and x 8192 envs (C5: 49,152 rows), the default schedule - the
    two-stream backward with dW row slices sized for half the CUs, the early reduction on the
    second stream, the K-specialised and half-tile forward instantiations - one epoch of 4
    minibatches, every coordinate of every step checked as in test_fused_update_every_step_is_exact
    (gradient vs autograd at the recorded parameters and rows, the step vs float64 clip + Adam)."""
    from ppo_trace import StepTrace, adam64, flat_view
    for var in ("LGX_GEMM_ALGO", "LGX_PPO_DW_SIDE", "LGX_PPO_EARLY_REDUCE", "LGX_PPO_SPLITS"):
        assert var not in os.environ, var     # the bench's default schedule
    Tb = 24
    ref, fus = make_pair("adaptive", None, T=Tb, N=n_envs, epochs=1)
    f = fus._fused
    tr = StepTrace(f)
    torch.manual_seed(11)
    fus.update()
    tr.close()
    assert f.M == Tb * n_envs // 4 and f.split and f.tn and f.loss_bwd and sorted(f.gemm_dw) == [0, 1, 2]
    assert getattr(f, "_side", None) is not None      # the dW GEMMs ran on the second stream
    assert f.Sk == [f._tn_slices(512, OBS, f.M, fill=0.5), f._tn_slices(256, 512, f.M, fill=0.5),
                    f._tn_slices(128, 256, f.M, fill=0.5)]
    torch.manual_seed(11)
    ref.update()
    assert fus.learning_rate == ref.learning_rate
    assert len(tr.steps) == 4
    params = list(ref.actor_critic.parameters())
    for t, rec in enumerate(tr.steps):
        with torch.no_grad():
            for p, q in zip(params, f.optimizer.params):
                off = f.off[id(q)]
                p.copy_(rec["p0"][off:off + q.numel()].view_as(p))
        g_ref = flat_view(f, list(autograd_grads(ref, rec["idx"]).values()))
        g = rec["g"].double()
        bad = ((g - g_ref).abs() > 1e-5 + 2e-3 * g_ref.abs()).sum().item()
        assert bad == 0, (n_envs, t, bad, (g - g_ref).abs().max().item())
        p_want, m_want, v_want = adam64(rec, fus.max_grad_norm)
        dp = (rec["p1"].double() - p_want).abs()
        assert (dp <= 1e-6 + 1e-3 * rec["lr"]).all(), (n_envs, t, dp.max().item(), rec["lr"])
        m_scale = 0.9 * rec["m0"].double().abs() + (m_want - 0.9 * rec["m0"].double()).abs()
        assert ((rec["m1"].double() - m_want).abs() <= 1e-5 * m_scale + 1e-12).all(), t
        assert ((rec["v1"].double() - v_want).abs() <= 2e-5 * v_want.abs() + 1e-18).all(), t
        if t > 0:
            assert torch.equal(rec["p0"], tr.steps[t - 1]["p1"])
