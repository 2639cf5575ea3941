"""GPU: the observation history written by the post-physics launch (lgx_bind_obs_history), against
tests/obs_history_ref.py - plain torch that replays the rule from the returned rows, reset_buf and
the explicit reset_idx calls.  The reference project has no observation history, so the rows are
pinned against this project's own layout.  Every comparison is bitwise: the tail
is a masked copy.

Episodes are a few steps long and start at random lengths, so time-outs stagger over the envs and
every age 0..H occurs; 37 envs are two full post-physics workgroups (16 envs each) and a 5-env tail.
"""
import ctypes as C

import pytest
import torch

from obs_history_ref import ObsHistoryRef
from oracle_backend import make_env

pytestmark = pytest.mark.gpu

EP_STEPS = 8      # episode length in steps (dt = 0.02 s)
ASYM_HIST = "go1_rough_asym_hist"      # Go1RoughAsymHistCfg, registered for the duration of a test


@pytest.fixture
def asym_hist_task():
    """Go1RoughAsymHistCfg (history + privileged critic: actor 475, critic 253) is a config class, not
    a registered task: register it under a name of the tests' own, and take it out again."""
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.envs.go1.go1_config import Go1RoughAsymHistCfg, Go1RoughCfgPPO
    from legged_gym_amd.utils.task_registry import task_registry
    task_registry.register(ASYM_HIST, Go1, Go1RoughAsymHistCfg(), Go1RoughCfgPPO())
    yield ASYM_HIST
    for d in (task_registry.task_classes, task_registry.env_cfgs, task_registry.train_cfgs):
        d.pop(ASYM_HIST, None)


def hist(frames, width=48, short_episodes=True, extra=None):
    def override(cfg):
        if frames is not None:
            cfg.history.frames, cfg.history.frame_width = frames, width
        if short_episodes:
            cfg.env.episode_length_s = EP_STEPS * 0.02
        if extra:
            extra(cfg)
    return override


def actions(k, n):
    g = torch.Generator().manual_seed(2000 + k)
    return ((torch.rand(n, 12, generator=g) - 0.5) * 2).cuda()


def stagger(env, seed=5):
    g = torch.Generator().manual_seed(seed)
    env.episode_length_buf = torch.randint(0, EP_STEPS, (env.num_envs,), generator=g)


def mismatch(got, want):
    bad = (got != want).nonzero()
    return [(i, j, got[i, j].item(), want[i, j].item()) for i, j in bad[:8].tolist()]


class Tracker:
    """The env's returned rows against the reference model, plus what the run covered."""

    def __init__(self, env):
        lay = env.history_layout
        self.env, self.nb = env, env.num_base_obs
        self.ref = ObsHistoryRef(env.num_envs, self.nb, lay.frames, lay.frame_width, device="cuda:0")
        self.resets, self.ages = 0, set()

    def reset_idx(self, ids):
        self.env.reset_idx(ids)
        self.ref.reset_idx(ids)

    def check(self, tag):
        env = self.env
        row = env.obs_buf
        assert row is env.get_observations() and row.shape == (env.num_envs, env.num_obs)
        base = env._obs_bufs[env._obs_slot]          # the kernel's own row (lgx_buffers.obs), unchanged
        assert torch.equal(row[:, :self.nb], base), (tag, mismatch(row[:, :self.nb], base))
        want = self.ref.step(row[:, :self.nb], env.reset_buf)
        assert torch.equal(row, want), (tag, mismatch(row, want))
        self.resets += int(env.reset_buf.sum())
        self.ages |= set(self.ref.last_a.tolist())
        return row


def make_tracked(task, n, frames, width=48, **kw):
    env = make_env(task, num_envs=n, device="cuda:0", backend="lgx", overrides=hist(frames, width, **kw))
    lay = env.history_layout
    assert (lay.frames, lay.frame_width) == (frames, width)
    assert env.num_obs == env.num_base_obs + frames * width == lay.width and env.obs_buf.shape == (n, lay.width)
    tr = Tracker(env)
    tr.ref.reset_idx(range(n))      # env.reset(): reset_idx on every env, then one zero-action step
    env.reset()
    tr.check("reset")
    assert not env.obs_buf[:, env.num_base_obs:].any(), "the first row of every episode has no past"
    stagger(env)
    return env, tr


@pytest.mark.parametrize("route", ["step", "post_physics", "post_physics_fused"])
def test_go1_rough_rows_are_bitwise_the_reference_model(gpu, route):
    """go1_rough (235 obs, the fused post-physics + actuator launch), H = 5, W = 48, 37 envs, 40
    launches: through env.step alone, and with every other launch a post_physics_step (the
    post-physics kernel alone / the fused launch) on the state the step left."""
    N, H = 37, 5
    env, tr = make_tracked("go1_rough", N, H)
    assert env.num_obs == 475
    for k in range(40):
        if route == "step" or k % 2 == 0:
            env.step(actions(k, N))
        else:
            env.post_physics_step(fused=route == "post_physics_fused")
        row = tr.check((route, k))
        assert row[:, :235].any(dim=1).all()
    # the run was not vacuous: in-step resets happened, and rows with a partial and a full history
    assert tr.resets >= N // 4 + 1, tr.resets
    assert any(0 < a < H for a in tr.ages) and H in tr.ages and 0 in tr.ages, tr.ages
    assert env.obs_buf[:, 235:].any(dim=0).all(), "every tail column carried data in the last row"


@pytest.mark.parametrize("task,frames,width,n", [("anymal_c_flat", 1, 48, 16), ("anymal_c_flat", 1, 48, 17),
                                                 ("anymal_c_flat", 9, 48, 16), ("anymal_c_flat", 9, 48, 17),
                                                 ("go1", 3, 45, 16), ("go1", 3, 45, 17)])
def test_shapes_where_indexing_can_go_wrong(gpu, task, frames, width, n):
    """48 observations on the plain post-physics kernel (anymal_c_flat: no actuator workgroups) with
    one frame and with nine (480 wide), go1 flat with frames of 45 (no multiple of 4: no row or frame
    is 16-byte aligned); one full workgroup of 16 envs, and 17."""
    env, tr = make_tracked(task, n, frames, width)
    assert env.num_base_obs == 48 and env.num_obs == 48 + frames * width
    for k in range(2 * EP_STEPS + frames + 2):
        env.step(actions(k, n))
        tr.check((task, frames, width, n, k))
    assert tr.resets >= n // 4 + 1 and frames in tr.ages and 0 in tr.ages, (tr.resets, tr.ages)


@pytest.mark.parametrize("base,with_history", [("go1_rough", ("go1_rough", 5)), ("go1_rough", ("go1_rough_hist", None)),
                                               ("go1_rough_asym", (ASYM_HIST, None))])
def test_nothing_else_moves_and_unbinding_restores_the_plain_env(gpu, asym_hist_task, base, with_history):
    """A same-seed env without a history: bitwise the same observations, rewards, resets, episode
    sums and privileged rows over the run; after lgx_bind_obs_history(NULL) the env goes on as the
    one that never bound a history, and the wide buffers are no longer written."""
    N = 37
    task, frames = with_history
    plain = make_env(base, num_envs=N, device="cuda:0", backend="lgx", overrides=hist(None))
    wide = make_env(task, num_envs=N, device="cuda:0", backend="lgx", overrides=hist(frames))
    assert plain.history_layout is None and plain.num_obs == 235 and wide.num_obs == 475
    assert (wide.privileged_obs_buf is None) == (plain.privileged_obs_buf is None) == (base == "go1_rough")
    for env in (plain, wide):
        env.reset()
        stagger(env)

    def same(k):
        a, b = plain.step(actions(k, N)), wide.step(actions(k, N))
        assert torch.equal(a[0], b[0][:, :235]), (k, mismatch(a[0], b[0][:, :235]))
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), k
        assert torch.equal(plain._episode_sums_buf, wide._episode_sums_buf), k
        assert torch.equal(plain.root_states, wide.root_states), k
        if a[1] is None:
            assert b[1] is None
        else:
            assert b[1].shape == (N, 253) and torch.equal(a[1], b[1]), (k, mismatch(a[1], b[1]))
        return a, b

    resets = 0
    for k in range(14):
        a, b = same(k)
        resets += int(a[3].sum())
    assert resets >= N // 4 + 1 and b[0][:, 235:].any()
    # unbind
    old = [t.clone() for t in wide._hist_bufs]
    bufs, wide._hist_bufs, wide.num_obs = wide._hist_bufs, None, wide.num_base_obs
    wide._backend.bind_obs_history(None, None, None)
    lib, h = wide._backend.lib, wide._backend.handle
    assert lib.lgx_rebind_obs_history(h, C.c_void_p(bufs[0].data_ptr()), C.c_void_p(bufs[1].data_ptr())) == -1
    assert b"no observation history is bound" in lib.lgx_last_error()
    for k in range(14, 20):
        a, b = same(k)
        assert b[0].shape == (N, 235)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(bufs, old))


def test_reset_idx_between_steps_clears_the_listed_envs_only(gpu):
    N, H = 17, 3
    env, tr = make_tracked("go1", N, H, short_episodes=False)
    for k in range(H + 2):
        env.step(actions(k, N))
        tr.check(k)
    assert not env.reset_buf.any() and tr.ages == set(range(H + 1))
    ids = [0, 5, 15, 16]
    rest = [e for e in range(N) if e not in ids]
    before = [b.clone() for b in env._hist_bufs]
    tr.reset_idx(torch.tensor(ids, device="cuda:0"))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(env._hist_bufs, before)), "reset_idx touches no row"
    prev = env.obs_buf
    env.step(actions(100, N))
    row = tr.check("after reset_idx")
    assert not env.reset_buf.any()
    assert not row[ids, 48:].any(), "their next tail is all zero"
    assert torch.equal(row[rest, 48:96], prev[rest, :48]) and torch.equal(row[rest, 96:], prev[rest, 48:144])
    assert row[rest, 48:].any(dim=1).all()
    env.step(actions(101, N))
    row = tr.check("second step after reset_idx")
    assert row[ids, 48:96].any(dim=1).all() and not row[ids, 96:].any()


def test_bind_validation_messages_and_the_width_limit(gpu):
    from legged_gym_amd.sim import abi
    N = 17
    env, tr = make_tracked("go1", N, 3, short_episodes=False)
    lib, h = env._backend.lib, env._backend.handle
    big = [torch.zeros(N, 513, device="cuda:0") for _ in range(2)]
    vp = lambda t: C.c_void_p(t.data_ptr())

    def bind(frames, fw, width, row=big[0], prev=big[1]):
        d = abi.LgxObsHistoryDesc(frames, fw, width)
        rc = lib.lgx_bind_obs_history(h, vp(row), vp(prev) if prev is not None else None, C.byref(d))
        return rc, lib.lgx_last_error().decode()

    for args, msg in (((0, 48, 48), "frames is below 1"), ((-1, 48, 0), "frames is below 1"),
                      ((2, 0, 48), "frame_width is outside [1, num_obs]"),
                      ((2, 49, 146), "frame_width is outside [1, num_obs]"),
                      ((2, 48, 143), "width is not num_obs + frames * frame_width"),
                      ((2, 48, 145), "width is not num_obs + frames * frame_width"),
                      ((31, 15, 513), "width is above LGX_MAX_PRIV_OBS"),
                      ((2, 48, 144, big[0], big[0]), "row and prev_row are the same buffer"),
                      ((2, 48, 144, big[0], None), "null prev_row")):
        rc, err = bind(*args)
        assert rc == -1 and "lgx_bind_obs_history: " + msg in err, (args[:3], rc, err)
    assert lib.lgx_bind_obs_history(h, vp(big[0]), vp(big[1]), None) == -1
    assert "lgx_bind_obs_history: null desc" in lib.lgx_last_error().decode()
    for row, prev, msg in ((None, big[1], "null argument"), (big[0], None, "null argument"),
                           (big[0], big[0], "row and prev_row are the same buffer")):
        assert lib.lgx_rebind_obs_history(h, vp(row) if row is not None else None,
                                          vp(prev) if prev is not None else None) == -1
        assert "lgx_rebind_obs_history: " + msg in lib.lgx_last_error().decode()
    # a refused bind leaves the bound history as it was
    for k in range(3):
        env.step(actions(k, N))
        tr.check(("after refused binds", k))
    # 512 is accepted (513 was refused above): 48 + 29 * 16.  The env's own buffers are narrower, so
    # the launches go through the backend here, not through env.step (which would rebind them).
    rc, err = bind(29, 16, 512)
    assert rc == 0, err
    wide = [b.view(-1)[:N * 512].view(N, 512) for b in big]
    counter = env.common_step_counter
    for k in range(3):          # a bind starts every env without a past
        assert lib.lgx_rebind_obs_history(h, vp(wide[k % 2]), vp(wide[(k + 1) % 2])) == 0
        env._backend.post_physics(counter + 1 + k)
        torch.cuda.synchronize()
        row, prev = wide[k % 2], wide[(k + 1) % 2]
        assert not env.reset_buf.any()
        assert torch.equal(row[:, :48], env._obs_bufs[env._obs_slot])
        assert torch.equal(row[:, 48:48 + 16 * k], torch.cat([prev[:, :16], prev[:, 48:]], dim=1)[:, :16 * k])
        assert not row[:, 48 + 16 * k:].any()
        assert k == 0 or row[:, 48:48 + 16 * k].any()
    assert all(not b.view(-1)[N * 512:].any() for b in big), "nothing past the 512-wide rows"
    env._backend.bind_obs_history(None, None, None)     # (the env's rebinds would no longer fit)
    env._hist_bufs = None


@pytest.mark.parametrize("task,cobs", [(ASYM_HIST, 253), ("go1_rough_hist", None)])
def test_go1_rough_hist_trains_one_iteration(gpu, asym_hist_task, task, cobs):
    """The history with the privileged critic (Go1RoughAsymHistCfg: actor 475, critic 253) and the
    registered go1_rough_hist (actor and critic read the 475-wide row), 64 envs x 8 steps, one OnPolicyRunner.learn iteration: the 475-wide rows in
    the storage are the rows env.step returned (the two buffers protect the tensor rsl_rl keeps
    until process_env_step), the rollout runs on the f32 MFMA forward, and the fused update matches
    the autograd PPO on the same storage, parameters and RNG - minibatch gradients and the whole
    update, to the tolerances tests/test_gpu_ppo.py uses for a privileged critic of another width."""
    from legged_gym_amd.envs.go1.go1_config import Go1RoughCfgPPO
    from legged_gym_amd.rl.actor_critic import ActorCritic
    from legged_gym_amd.rl.fused_ppo import FusedPPOUpdate
    from legged_gym_amd.rl.ppo import PPO
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    from test_gpu_ppo import autograd_grads
    N, T = 64, 8
    env = make_env(task, num_envs=N, device="cuda:0", backend="lgx")
    assert (env.num_obs, env.num_base_obs, env.num_privileged_obs) == (475, 235, cobs)
    cfg = class_to_dict(Go1RoughCfgPPO())
    cfg["runner"]["num_steps_per_env"] = T
    cfg["algorithm"]["num_learning_epochs"] = 2          # 8 Adam steps, as the update test of test_gpu_ppo.py
    torch.manual_seed(0)
    runner = OnPolicyRunner(env, cfg, None, device="cuda:0")
    alg = runner.alg
    ac = alg.actor_critic
    assert ac.actor[0].in_features == 475 and ac.critic[0].in_features == (cobs or 475)
    assert FusedPPOUpdate.supported(ac) and alg._fused is not None
    rec = {"returned": [env.get_observations().clone()], "resets": 0, "fused_act": [], "x3": []}
    orig_act, orig_step, orig_update = alg.act, env.step, alg.update

    def act(obs, cobs):
        out = orig_act(obs, cobs)
        rec["fused_act"].append(alg.last_act_fused)
        rec["x3"].append(ac._fused_actor.last_x3)
        return out

    def env_step(a):
        out = orig_step(a)
        rec["returned"].append(out[0].clone())
        rec["resets"] += int(out[3].sum())
        return out

    def update(defer=False):
        alg.flush_store()
        st = alg.storage
        rec["storage"] = st.observations.clone()
        # the autograd twin: same parameters, same storage
        twin = ActorCritic(475, cobs or 475, env.num_actions, **cfg["policy"]).to("cuda:0")
        twin.load_state_dict(ac.state_dict())
        ref = PPO(twin, device="cuda:0", use_fused_update=False, **cfg["algorithm"])
        ref.init_storage(N, T, [475], [cobs], [env.num_actions])
        for name in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob", "mu", "sigma",
                     "returns", "advantages") + (("privileged_observations",) if cobs else ()):
            getattr(ref.storage, name).copy_(getattr(st, name))
        ref.storage.step = st.step
        idx = torch.randperm(T * N, device="cuda:0")[: T * N // 4]
        gref = autograd_grads(ref, idx)
        alg._fused.gradients(idx)
        worst = 0.0
        for n, p in ac.named_parameters():
            a, b = p.grad, gref[n]
            worst = max(worst, ((a - b).abs() - 2e-3 * b.abs()).max().item())
        print(f"minibatch gradient: max(|d| - 2e-3 |g|) = {worst:.3e} (bound 1e-5)")
        for n, p in ac.named_parameters():
            a, b = p.grad, gref[n]
            assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), n
        torch.manual_seed(11)
        rec["ref_losses"] = ref.update()
        rec["ref"] = ref
        torch.manual_seed(11)
        return orig_update(defer=defer)     # (deferred readback: the runner resolves it)

    alg.act, env.step, alg.update = act, env_step, update
    runner.learn(1, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    # 475-wide rows do not fit the split-bf16 rollout kernel's LDS (lgx_mlp_x3_lds_bytes: decided on
    # the host from the widths alone), so act() is the f32 MFMA forward of both networks in one
    # launch (lgx_mlp_forward_batch) and lgx_ppo_act(_store) - HIP kernels, not the one fused launch
    assert len(rec["returned"]) == T + 1 and len(rec["x3"]) == T
    assert not any(rec["x3"]) and not any(rec["fused_act"]), (rec["x3"], rec["fused_act"])
    for t in range(T):
        # the row the actor acted on at step t is the row the previous env.step returned, and the
        # next env.step did not touch it before the storage copied it
        assert torch.equal(rec["storage"][t], rec["returned"][t]), t
    assert any(r[:, 235:].any() for r in rec["returned"]), "the rows carry a history"
    ref = rec["ref"]
    stats = runner.last_iteration_stats
    (vl_f, sl_f), (vl_r, sl_r) = (stats["value_loss"], stats["surrogate_loss"]), rec["ref_losses"]
    big = total = 0
    for (n, a), b in zip(ac.named_parameters(), ref.actor_critic.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    print(f"update: lr {alg.learning_rate} / {ref.learning_rate}, value loss {vl_f} / {vl_r}, surrogate {sl_f} / "
          f"{sl_r}, coordinates off by more than 1e-5: {big} of {total}")
    assert alg.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6
    assert big <= 1e-3 * total, (big, total)
    for name, p in ac.named_parameters():
        assert torch.isfinite(p).all(), name
