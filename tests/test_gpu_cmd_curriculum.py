"""GPU: the command curriculum on the device (lgx_bind_command_curriculum) against
tests/cmd_curriculum_ref.py, the numpy float64 restatement of the reference's rule.

37 envs are two full post-physics workgroups (16 envs each) and a tail of 5; episodes are L = 8
steps (episode_length_s = 0.159: in float64 8 * 0.02 / 0.02 is 8.000000000000002, whose ceil is 9).
State is scripted through the env's public tensors: `episode_sums["tracking_lin_vel"]`,
`episode_length_buf` (L: the env times out in the probe launch), `common_step_counter`.  The probe
launch adds this step's reward to the sums before it reduces them, so the scripted envs move at
60 m/s: exp(-58^2 / 0.25) is 0 in float32 and the sums stay what the script wrote.  The sums are
small multiples of 2^-7, so every summation order gives the same float32; 1.25 x and 0.75 x of
float32(0.016) * 8 are not such multiples, the cases sit just beyond them (>= 1.28 x, <= 0.74 x).
"""
import numpy as np
import pytest
import torch

import cmd_curriculum_ref as ref
from oracle_backend import make_env

pytestmark = pytest.mark.gpu

N = 37
L = 8                      # episode length in steps (dt = 0.02 s)
EPISODE_S = 0.159          # ceil(0.159 / 0.02) = 8
Q = 2.0 ** -7              # the scripted sums' unit
ABOVE = (21, 22, 23)       # x Q: mean / (thr * L) >= 1.28
BELOW = (10, 11, 12)       # x Q: mean / (thr * L) <= 0.74
SPREAD = [0, 5, 16, 17, 30, 36]          # reset envs in all three workgroups
ASYM_HIST = "go1_rough_asym_hist_cmdcur"


def cur(lo=0.5, max_c=1.0, on=True, extra=None):
    def override(cfg):
        cfg.commands.curriculum = on
        cfg.commands.max_curriculum = max_c
        cfg.commands.ranges.lin_vel_x = [-lo, lo]
        cfg.env.episode_length_s = EPISODE_S
        if extra:
            extra(cfg)
    return override


def short_resampling(cfg):
    cfg.commands.resampling_time = 0.09      # int(0.09 / 0.02) = 4 steps


def make(task="go1", **kw):
    env = make_env(task, num_envs=N, device="cuda:0", backend="lgx", overrides=cur(**kw))
    assert env.max_episode_length == L
    return env


def sums_of(ids, ks):
    s = np.zeros(N)
    for i, e in enumerate(ids):
        s[e] = ks[i % len(ks)] * Q
    return s


def script(env, reset_ids, sums, counter, resample_ids=()):
    """Leave `env` so that the next post-physics launch is step `counter`, resets exactly `reset_ids`
    (time-outs) and reduces exactly `sums` for them."""
    ep = torch.zeros(N, dtype=torch.long)
    ep[list(reset_ids)] = L
    ep[list(resample_ids)] = 3
    env.episode_length_buf = ep
    env.episode_sums["tracking_lin_vel"].copy_(torch.as_tensor(sums, dtype=torch.float32))
    env.contact_forces.zero_()                                   # nobody terminates on a contact
    env.root_states[:, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda:0")
    env.root_states[:, 7:10] = torch.tensor([60.0, 0.0, 0.0], device="cuda:0")
    env.common_step_counter = counter - 1


def state_of(env):
    torch.cuda.synchronize()
    return env.command_curriculum_state.cpu().numpy().astype(np.float64)


def probe(env, reset_ids, sums, counter, max_c=1.0, route="post_physics"):
    """One scripted launch; state against the ref.  Returns (state before, state after)."""
    before = state_of(env)
    script(env, reset_ids, sums, counter)
    if route == "post_physics":
        env.post_physics_step()
    elif route == "post_physics_fused":
        env.post_physics_step(fused=True)
    else:
        env.step(torch.zeros(N, 12, device="cuda:0"))
    after = state_of(env)
    assert sorted(env.reset_buf.nonzero().flatten().tolist()) == sorted(reset_ids)
    lo, hi, cnt, left = ref.decide(before[0], before[1], before[2], np.asarray(sums)[list(reset_ids)], counter, L,
                                   env.reward_scales["tracking_lin_vel"], max_c)
    print(f"counter {counter} resets {len(reset_ids)}: state {after.tolist()} ref {(lo, hi, cnt, left)}")
    assert after[:3].tolist() == [lo, hi, cnt]
    if left is None:
        assert after[3] == before[3]
    else:   # float32 summation of n non-negative terms, the mean's and the length's division
        assert abs(after[3] - left) <= (len(reset_ids) + 2) * 2.0 ** -24 * left
    return before, after


def restart(env, lo=0.5):
    env.set_command_range("lin_vel_x", -lo, lo)


def test_widens_and_only_then(gpu):
    env = make()
    env.reset()
    assert state_of(env).tolist() == [-0.5, 0.5, 0.0, 0.0]     # construction and reset(): counter 0, sums 0
    thr = float(np.float32(0.8 * env.reward_scales["tracking_lin_vel"]))
    assert min(ABOVE) * Q / (thr * L) >= 1.25 and max(BELOW) * Q / (thr * L) <= 0.75
    _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), L)
    assert a[:3].tolist() == [-1.0, 1.0, 1.0]                  # (fails without the feature: the range never moves)
    restart(env)
    _, a = probe(env, SPREAD, sums_of(SPREAD, BELOW), L)
    assert a[:2].tolist() == [-0.5, 0.5]
    for counter in (L - 1, L + 1, 3 * L + 5):                  # good tracking, but not a curriculum step
        _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), counter)
        assert a[:2].tolist() == [-0.5, 0.5]
    _, a = probe(env, [], sums_of(range(N), ABOVE), L)         # a curriculum step on which no env resets
    assert a[:2].tolist() == [-0.5, 0.5]
    _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), 5 * L)   # a later multiple
    assert a[:2].tolist() == [-1.0, 1.0]
    _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), 6 * L)   # at the bound: stays, and is not counted
    assert a[:2].tolist() == [-1.0, 1.0]
    # the published commands of the envs that reset: obs columns 9, 10 are commands * obs_scales.lin_vel
    assert torch.equal(env.obs_buf[:, 9:11], env.commands[:, :2] * env.obs_scales.lin_vel)


def test_clip_sequence_and_start_outside_the_interval(gpu):
    env = make(lo=0.3, max_c=1.0)
    env.reset()
    want = [(-0.8, 0.8), (-1.0, 1.0), (-1.0, 1.0)]
    for k, w in enumerate(want):
        _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), (k + 1) * L)
        assert np.allclose(a[:2], w, rtol=0, atol=1e-7) and a[:2].astype(np.float32).tolist() == list(np.float32(w))
    env.set_command_range("lin_vel_x", -2.0, 2.0)              # outside [-max, 0] / [0, max]: np.clip pulls it in
    _, a = probe(env, SPREAD, sums_of(SPREAD, ABOVE), 4 * L)
    assert a[:2].tolist() == [-1.0, 1.0]


@pytest.mark.parametrize("ids", [[16, 19, 31, 32, 36], [3, 20, 34], list(range(16, N))],
                         ids=["second-and-tail", "one-per-block", "all-of-second-and-tail"])
def test_cross_block_reduction(gpu, ids):
    env = make()
    env.reset()
    sums = sums_of(ids, (21, 30, 27, 44, 23))
    sums[[e for e in range(N) if e not in ids]] = 1000 * Q     # envs that do not reset must not count
    _, a = probe(env, ids, sums, L)
    assert a[:3].tolist() == [-1.0, 1.0, 1.0]
    restart(env)
    low = sums_of(ids, BELOW)
    low[[e for e in range(N) if e not in ids]] = 1000 * Q
    _, a = probe(env, ids, low, 2 * L)
    assert a[:2].tolist() == [-0.5, 0.5]


def test_strict_inequality(gpu):
    """Four reset envs with identical sums s = thr * L, two in each of two workgroups (s + s and
    2s + 2s are exact): the left side is the threshold itself, which is not greater.  The next
    float32 above it is."""
    env = make()
    env.reset()
    thr = np.float32(0.8 * env.reward_scales["tracking_lin_vel"])
    ids = [0, 1, 16, 17]
    s = np.zeros(N)
    s[ids] = float(thr) * L
    _, a = probe(env, ids, s, L)
    assert a[:3].tolist() == [-0.5, 0.5, 0.0] and np.float32(a[3]) == thr
    s[ids] = float(np.nextafter(thr, np.float32(1))) * L
    _, a = probe(env, ids, s, 2 * L)
    assert a[:3].tolist() == [-1.0, 1.0, 1.0] and np.float32(a[3]) == np.nextafter(thr, np.float32(1))


# ------------------------------------------------------------------ the same-step resample
@pytest.fixture
def asym_hist_task():
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.envs.go1.go1_config import Go1RoughAsymHistCfg, Go1RoughCfgPPO
    from legged_gym_amd.utils.task_registry import task_registry
    task_registry.register(ASYM_HIST, Go1, Go1RoughAsymHistCfg(), Go1RoughCfgPPO())
    yield ASYM_HIST
    for d in (task_registry.task_classes, task_registry.env_cfgs, task_registry.train_cfgs):
        d.pop(ASYM_HIST, None)


def history5(cfg):
    cfg.history.frames = 5


PUBLIC_STATE = ("root_states", "dof_state", "commands", "actions", "last_actions", "last_dof_vel", "last_root_vel",
                "_feet_air_time_full", "_episode_sums_buf", "torques", "_contact_forces_full", "env_origins",
                "terrain_levels", "base_lin_vel", "base_ang_vel", "projected_gravity")


def actions(k):
    g = torch.Generator().manual_seed(4000 + k)
    return ((torch.rand(N, 12, generator=g) - 0.5) * 0.5).cuda()


@pytest.mark.parametrize("route", ["post_physics", "post_physics_fused", "step"])
@pytest.mark.parametrize("task", ["go1", "go1_rough_hist5", "asym_hist"])
def test_same_step_resample_is_bitwise_a_launch_on_the_new_range(gpu, route, task, asym_hist_task):
    """A widens in the probe launch and patches the envs that reset; B, in the same state, already
    holds the widened range (its decision clips to "no change"), so its launch samples from it by
    itself.  Everything both publish must be equal."""
    name, extra = {"go1": ("go1", None), "go1_rough_hist5": ("go1_rough", history5),
                   "asym_hist": (asym_hist_task, None)}[task]
    A, B = make(name, extra=extra), make(name, extra=extra)
    for env in (A, B):
        env.reset()
        for k in range(3):                          # the same launches: the history ages agree
            env.step(actions(k))
    for f in PUBLIC_STATE:
        getattr(B, f).copy_(getattr(A, f))
    resets = [1, 2, 7, 15, 16, 18, 21, 29, 31, 32, 33, 36]
    ep = torch.tensor([(3 * e) % 5 for e in range(N)])      # forced time-outs do not depend on commands
    ep[resets] = L
    for env in (A, B):
        env.episode_length_buf = ep
        env.episode_sums["tracking_lin_vel"].fill_(64 * Q)
        env.common_step_counter = L - 1
    B.set_command_range("lin_vel_x", -1.0, 1.0)
    for env in (A, B):
        if route == "step":
            env.step(actions(9))
        else:
            env.post_physics_step(fused=route == "post_physics_fused")
    sa, sb = state_of(A), state_of(B)
    print(f"{task} {route}: A {sa.tolist()} B {sb.tolist()} resets {int(A.reset_buf.sum())}")
    assert sa[:3].tolist() == [-1.0, 1.0, 1.0] and sb[:3].tolist() == [-1.0, 1.0, 0.0] and sa[3] == sb[3]
    assert A.reset_buf[resets].all() and torch.equal(A.reset_buf, B.reset_buf)
    assert torch.equal(A.commands, B.commands)
    assert (A.commands[resets, 0].abs() > 0.5).any(), "no reset env drew beyond the old range: the probe shows nothing"
    assert torch.equal(A.rew_buf, B.rew_buf)
    assert torch.equal(A.obs_buf, B.obs_buf)                     # the wide row where a history is bound
    assert torch.equal(A._obs_bufs[A._obs_slot], B._obs_bufs[B._obs_slot])
    if task != "go1":
        assert A.obs_buf.shape[1] == A.num_base_obs + 5 * 48
    if task == "asym_hist":
        assert A.privileged_obs_buf.shape[1] == 253
        assert torch.equal(A.privileged_obs_buf, B.privileged_obs_buf)


def dyadic_draws(env):
    """Injected draws, every one a small dyadic fraction (float32 arithmetic on them is exact):
    0.5 everywhere (no noise, no offset), the periodic resample's x, y = 0.875, 0.125, the reset's
    x per env in {1/16, 3/16, ..., 15/16} and y = 0.75."""
    d = torch.full((N, ref.DRAW_NOISE + env.num_base_obs), 0.5)
    d[:, ref.DRAW_CMD], d[:, ref.DRAW_CMD + 1] = 0.875, 0.125
    d[:, ref.DRAW_RESET_CMD] = (2 * (torch.arange(N) % 8) + 1) / 16.0
    d[:, ref.DRAW_RESET_CMD + 1] = 0.75
    return d


def f32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32)


def test_interval_resamples_keep_the_old_range(gpu):
    """Envs that only hit resample_interval in the probe step drew from the old range (that resample
    runs before reset_idx); the envs that reset draw from the new one."""
    env = make(extra=short_resampling)
    env.reset()
    d = dyadic_draws(env)
    dev = d.cuda()
    env._backend.set_draws(dev)
    resets, resample = [0, 5, 16, 17, 30, 36], [2, 3, 20, 35]
    script(env, resets, sums_of(resets, ABOVE), L, resample_ids=resample)
    before = env.commands.clone()
    env.post_physics_step()
    a = state_of(env)
    assert a[:3].tolist() == [-1.0, 1.0, 1.0]
    ry = env.command_ranges["lin_vel_y"]
    got = env.commands.cpu()
    cx, cy = ref.draw_xy(d[resample, ref.DRAW_CMD], d[resample, ref.DRAW_CMD + 1], (-0.5, 0.5), ry)
    assert torch.equal(got[resample, 0], f32(cx)) and torch.equal(got[resample, 1], f32(cy))
    assert cx.tolist() == [0.375] * 4                                        # (1.0 - 0.5 would be 0.75)
    cx, cy = ref.draw_xy(d[resets, ref.DRAW_RESET_CMD], d[resets, ref.DRAW_RESET_CMD + 1], (-1.0, 1.0), ry)
    assert torch.equal(got[resets, 0], f32(cx)) and torch.equal(got[resets, 1], f32(cy))
    rest = [e for e in range(N) if e not in resets + resample]
    assert torch.equal(got[rest, :2], before.cpu()[rest, :2])
    assert torch.equal(env.obs_buf[:, 9:11], env.commands[:, :2] * env.obs_scales.lin_vel)
    env._backend.set_draws(None)


def test_next_launches_read_the_new_range(gpu):
    """After a widening, ordinary steps sample from the new range: with draws of 1.0 the periodic
    resample gives x = hi_new exactly - also three steps later, each of which rebinds obs and extras."""
    env = make(extra=short_resampling)
    env.reset()
    d = torch.full((N, ref.DRAW_NOISE + env.num_base_obs), 0.5)
    for slot in (ref.DRAW_CMD, ref.DRAW_CMD + 1, ref.DRAW_RESET_CMD, ref.DRAW_RESET_CMD + 1):
        d[:, slot] = 1.0
    dev = d.cuda()
    env._backend.set_draws(dev)
    everyone = list(range(N))
    script(env, everyone, sums_of(everyone, ABOVE), L)
    env.post_physics_step()                       # widens; every env resets (and leaves the 60 m/s behind)
    assert state_of(env)[:3].tolist() == [-1.0, 1.0, 1.0]
    hi_new = float(ref.draw_xy(1.0, 1.0, (-1.0, 1.0), env.command_ranges["lin_vel_y"])[0])
    assert hi_new == 1.0
    for k in range(4):
        env.episode_length_buf = torch.full((N,), 3)          # ep = 4: the interval, no time-out
        env.step(torch.zeros(N, 12, device="cuda:0"))
        assert not ref.is_curriculum_step(env.common_step_counter, L)
        torch.cuda.synchronize()
        assert (env.commands[:, 0] == hi_new).all(), (k, env.commands[:, 0].tolist())
    env._backend.set_draws(None)


def test_reset_idx_route(gpu):
    env = make()
    env.reset()
    d = dyadic_draws(env)
    dev = d.cuda()
    env._backend.set_draws(dev)
    ids = [1, 17, 18, 35]
    ry = env.command_ranges["lin_vel_y"]

    def run(counter, sums):
        env.episode_sums["tracking_lin_vel"].copy_(f32(sums))
        env.common_step_counter = counter
        before = [b.clone() for b in env._obs_bufs] + [env.commands.clone()]
        env.reset_idx(ids)
        torch.cuda.synchronize()
        assert all(torch.equal(b, c) for b, c in zip(env._obs_bufs, before)), "reset_idx touches no observation row"
        rest = [e for e in range(N) if e not in ids]
        assert torch.equal(env.commands[rest], before[2][rest])
        return env.commands.cpu()[ids, :2]

    sums = sums_of(ids, ABOVE)
    got = run(L + 1, sums)                                       # not a curriculum step: the old range
    assert state_of(env)[:3].tolist() == [-0.5, 0.5, 0.0]
    cx, cy = ref.draw_xy(d[ids, ref.DRAW_RESET_CMD], d[ids, ref.DRAW_RESET_CMD + 1], (-0.5, 0.5), ry)
    assert torch.equal(got, torch.stack([f32(cx), f32(cy)], 1))
    got = run(L, sums)
    a = state_of(env)
    want = ref.decide(-0.5, 0.5, 0, sums[ids], L, L, env.reward_scales["tracking_lin_vel"], 1.0)
    assert a[:3].tolist() == list(want[:3]) == [-1.0, 1.0, 1.0]
    assert abs(a[3] - want[3]) <= (len(ids) + 2) * 2.0 ** -24 * want[3]
    cx, cy = ref.draw_xy(d[ids, ref.DRAW_RESET_CMD], d[ids, ref.DRAW_RESET_CMD + 1], (-1.0, 1.0), ry)
    assert torch.equal(got, torch.stack([f32(cx), f32(cy)], 1))
    env._backend.set_draws(None)


# ------------------------------------------------------------------ surface
def test_max_command_x_and_sync(gpu):
    env = make()
    env.reset()
    t0 = env.extras["episode"]["max_command_x"]
    assert t0.device.type == "cuda" and t0.dim() == 0 and t0.item() == 0.5
    env.step(torch.zeros(N, 12, device="cuda:0"))
    assert env.extras["episode"]["max_command_x"] is t0          # no curriculum step: the same tensor
    everyone = list(range(N))
    script(env, everyone, sums_of(everyone, ABOVE), L)
    env.post_physics_step()
    t1 = env.extras["episode"]["max_command_x"]
    assert t1 is not t0 and t1.item() == 1.0 == env.command_curriculum_state[1].item() and t0.item() == 0.5
    env.step(torch.zeros(N, 12, device="cuda:0"))
    assert env.extras["episode"]["max_command_x"] is t1
    assert env.command_ranges["lin_vel_x"] == [-0.5, 0.5]        # the host copy, until an explicit sync
    assert env.sync_command_ranges()["lin_vel_x"] == [-1.0, 1.0]
    env.set_command_range("lin_vel_x", -0.25, 0.75)
    assert state_of(env)[:2].tolist() == [-0.25, 0.75] and env.command_ranges["lin_vel_x"] == [-0.25, 0.75]
    env.step(torch.zeros(N, 12, device="cuda:0"))
    assert env.extras["episode"]["max_command_x"].item() == 0.75


def test_cmdcur_task_runs(gpu):
    def short(cfg):
        cfg.env.episode_length_s = EPISODE_S
    env = make_env("go1_rough_cmdcur", num_envs=N, device="cuda:0", backend="lgx", overrides=short)
    assert state_of(env).tolist() == [-0.5, 0.5, 0.0, 0.0] and env.cfg.commands.max_curriculum == 1.0
    env.reset()
    for k in range(2 * L):
        obs, _, rew, _, extras = env.step(actions(k))
    a = state_of(env)
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all() and np.isfinite(a).all()
    assert a[:2].tolist() in ([-0.5, 0.5], [-1.0, 1.0]) and a[3] >= 0
    assert extras["episode"]["max_command_x"].item() == a[1]


def test_library_refusals(gpu, monkeypatch):
    from legged_gym_amd.envs.base.legged_robot import LeggedRobot
    from legged_gym_amd.sim.lib import LgxError

    def no_tracking(cfg):
        cfg.rewards.scales.tracking_lin_vel = 0.0
    state = torch.zeros(4, device="cuda:0")
    env = make(on=False, extra=no_tracking)
    with pytest.raises(LgxError, match="tracking_lin_vel"):
        env._backend.bind_command_curriculum(state, 1.0, 0.016)
    with pytest.raises(ValueError, match="tracking_lin_vel"):
        make(extra=no_tracking)

    orig = LeggedRobot._get_noise_scale_vec

    def noisy_commands(self, cfg):
        nv = orig(self, cfg)
        nv[9:12] = 0.05
        return nv
    monkeypatch.setattr(LeggedRobot, "_get_noise_scale_vec", noisy_commands)
    env = make(on=False)
    with pytest.raises(LgxError, match="noise_scale_vec"):
        env._backend.bind_command_curriculum(state, 1.0, 0.016)
    with pytest.raises(ValueError, match="noise_scale_vec"):
        make()
    monkeypatch.undo()
    env = make(on=False)
    with pytest.raises(LgxError, match="max_curriculum"):
        env._backend.bind_command_curriculum(state, -1.0, 0.016)
    with pytest.raises(LgxError, match="lgx_set_command_range"):
        env._backend.set_command_range(4, 0.0, 1.0)
    with pytest.raises(LgxError, match="lo <= hi"):
        env._backend.set_command_range(0, 1.0, -1.0)
    env._backend.bind_command_curriculum(state, 1.0, 0.016)      # a valid bind, and the unbind
    torch.cuda.synchronize()
    assert state.tolist() == [-0.5, 0.5, 0.0, 0.0]
    env._backend.bind_command_curriculum(None, 0.0, 0.0)


def test_switch_off_binds_nothing(gpu):
    """commands.curriculum = False: nothing is bound, the surface is the parent's, and a 2 L-step run
    is reproducible bit for bit on commands and obs."""
    A, B = make(on=False), make(on=False)
    for env in (A, B):
        assert env.command_curriculum_state is None
        env.reset()
        assert "max_command_x" not in env.extras["episode"]
    for k in range(2 * L):
        oa = A.step(actions(k))[0]
        ob = B.step(actions(k))[0]
        assert torch.equal(oa, ob) and torch.equal(A.commands, B.commands), k
    assert A.sync_command_ranges()["lin_vel_x"] == [-0.5, 0.5]
