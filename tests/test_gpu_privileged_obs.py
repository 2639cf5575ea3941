"""GPU: the privileged observation row written by the post-physics launch (lgx_bind_privileged_obs),
against tests/privileged_obs_ref.py - plain torch over the env's public tensors after each step.
The reference project never fills its privileged buffer, so the row is pinned against this
project's own layout, not against reference semantics.

N = 35 envs: two full post-physics workgroups (16 envs each) and a 3-env tail.  Row widths are
not multiples of 4 (48 + 43 = 91, 235 + 43 = 278, 235 + 18 = 253), so rows are not 16-byte aligned.
"""
import ctypes as C

import pytest
import torch

from oracle_backend import make_env
from privileged_obs_ref import privileged_obs_ref

pytestmark = pytest.mark.gpu

N = 35
STEPS = 30
ALL_TERMS = ("friction", "base_mass", "mass_scale", "feet_contact", "feet_forces", "torques")
FORCED = [0, 15, 16, 34]      # first / last env of a workgroup, and the last env of the tail


def asym(terms=ALL_TERMS, add_noise=None, privileged=True):
    def override(cfg):
        if privileged:
            from legged_gym_amd.envs.base.privileged import layout
            cfg.privileged.terms = tuple(terms)
            cfg.env.num_privileged_obs = layout(terms, cfg.env.num_observations, 4).width
        if add_noise is not None:
            cfg.noise.add_noise = add_noise
    return override


def actions(k):
    g = torch.Generator().manual_seed(1000 + k)
    return ((torch.rand(N, 12, generator=g) - 0.5) * 2).cuda()


def force_reset(env, ids=FORCED):
    env._episode_length_buf[torch.tensor(ids, device=env.device)] = int(env.max_episode_length) + 1


def mismatch(got, want):
    bad = (got != want).nonzero()
    return [(i, j, got[i, j].item(), want[i, j].item()) for i, j in bad[:8].tolist()]


@pytest.mark.parametrize("task,act_overlap", [("go1", None), ("go1_rough", None), ("go1_rough", "1")])
def test_row_is_bitwise_the_torch_reference_on_every_route(gpu, monkeypatch, task, act_overlap):
    """All six terms behind 48 / 235 clean entries (235: the last quad of a row is partial), through
    step() (post-physics + actuator net in one launch), post_physics_step(fused=False) (the
    post-physics kernel alone) and post_physics_step(fused=True); LGX_ACT_OVERLAP=1 sends step()
    through the separate-launch path.  Every entry is one float32 subtract and one multiply: bitwise."""
    if act_overlap is not None:
        monkeypatch.setenv("LGX_ACT_OVERLAP", act_overlap)
    env = make_env(task, num_envs=N, device="cuda:0", backend="lgx", overrides=asym())
    assert env.num_privileged_obs == env.num_obs + 43 and env.num_privileged_obs % 4 != 0
    resets = 0
    seen = torch.zeros(43, dtype=torch.bool, device="cuda:0")
    for k in range(STEPS):
        routes = [lambda: env.step(actions(k))]
        if k % 3 == 2:
            routes += [lambda: env.post_physics_step(fused=False), lambda: env.post_physics_step(fused=True)]
        for r, route in enumerate(routes):
            if (k, r) in ((7, 0), (11, 1), (20, 2)):
                force_reset(env)
            route()
            if (k, r) in ((7, 0), (11, 1), (20, 2)):
                assert env.reset_buf[FORCED].all()
            resets += int(env.reset_buf.sum())
            got, want = env.get_privileged_observations(), privileged_obs_ref(env)
            assert got.shape == want.shape == (N, env.num_privileged_obs)
            assert torch.equal(got, want), (k, r, mismatch(got, want))
            seen |= (got[:, env.num_obs:] != 0).any(dim=0)
    assert resets >= 3 * len(FORCED)
    assert seen.all(), ("a tail column that never carried data", (~seen).nonzero().flatten().tolist())


def test_noise_off_clean_part_is_the_observation(gpu):
    env = make_env("go1_rough", num_envs=N, device="cuda:0", backend="lgx", overrides=asym(add_noise=False))
    for k in range(STEPS):
        if k == 9:
            force_reset(env)
        obs, priv, *_ = env.step(actions(k))
        assert torch.equal(priv[:, :env.num_obs], obs), (k, mismatch(priv[:, :env.num_obs], obs))


def test_noise_on_clean_part_is_the_noise_free_trajectory(gpu):
    """|obs - clean| <= noise_scale_vec (1 + 1e-6) where neither side was clipped, the two differ in
    every env, and a twin env without noise (same seed, same actions: the noise slots are Philox
    blocks of their own, so the trajectory does not depend on them) has obs bitwise equal to the
    noisy env's clean part."""
    noisy = make_env("go1_rough", num_envs=N, device="cuda:0", backend="lgx", overrides=asym(add_noise=True))
    twin = make_env("go1_rough", num_envs=N, device="cuda:0", backend="lgx", overrides=asym(add_noise=False,
                                                                                            privileged=False))
    assert twin.privileged_obs_buf is None
    no, clip = noisy.num_obs, noisy.cfg.normalization.clip_observations
    bound = noisy.noise_scale_vec.double() * (1 + 1e-6)
    assert (bound > 0).sum() == no - 15            # commands (3) and actions (12) carry no noise
    for k in range(STEPS):
        if k == 9:
            force_reset(noisy)
            force_reset(twin)
        obs, priv, *_ = noisy.step(actions(k))
        tobs = twin.step(actions(k))[0]
        clean = priv[:, :no]
        free = (obs.abs() < clip) & (clean.abs() < clip)
        diff = (obs.double() - clean.double()).abs()
        over = (diff > bound) & free
        assert not over.any(), (k, over.nonzero()[:8].tolist(), diff[over][:8].tolist())
        assert (obs != clean).any(dim=1).all(), k
        assert torch.equal(tobs, clean), (k, mismatch(tobs, clean))


def test_feature_off_changes_nothing(gpu):
    """An env without num_privileged_obs and one with the row bound: bitwise the same obs, rewards,
    resets and episode sums over the run (passes without the feature too, by design)."""
    plain = make_env("go1_rough", num_envs=N, device="cuda:0", backend="lgx")
    bound = make_env("go1_rough", num_envs=N, device="cuda:0", backend="lgx", overrides=asym())
    assert plain.privileged_obs_buf is None and plain.get_privileged_observations() is None
    assert plain.add_noise and bound.add_noise
    for k in range(STEPS):
        if k == 9:
            force_reset(plain)
            force_reset(bound)
        a, b = plain.step(actions(k)), bound.step(actions(k))
        assert a[1] is None
        assert torch.equal(a[0], b[0]), (k, mismatch(a[0], b[0]))
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), k
        assert torch.equal(plain._episode_sums_buf, bound._episode_sums_buf), k
        assert torch.equal(plain.root_states, bound.root_states), k


def test_rows_are_double_buffered(gpu):
    env = make_env("go1", num_envs=N, device="cuda:0", backend="lgx", overrides=asym())
    _, prev, *_ = env.step(actions(0))
    for k in range(1, 6):
        keep = prev.clone()
        _, cur, *_ = env.step(actions(k))
        assert cur.data_ptr() != prev.data_ptr()
        assert torch.equal(prev, keep), "the row step k returned is unchanged after step k + 1"
        assert not torch.equal(cur, keep)
        assert env.get_privileged_observations() is cur and env.privileged_obs_buf is cur
        assert torch.equal(cur, privileged_obs_ref(env))
        prev = cur
    _, first = env.reset()
    assert first is env.get_privileged_observations() and torch.equal(first, privileged_obs_ref(env))


def test_bind_validation_and_unbind(gpu):
    from legged_gym_amd.sim import abi
    env = make_env("go1", num_envs=N, device="cuda:0", backend="lgx", overrides=asym())
    lib, h = env._backend.lib, env._backend.handle
    buf = torch.zeros(N, 512, device="cuda:0")

    def bind(width, ids=(), offs=()):
        d = abi.LgxPrivObsDesc()
        d.width, d.num_terms = width, len(ids)
        for t, (i, o) in enumerate(zip(ids, offs)):
            d.term_ids[t], d.term_offsets[t] = i, o
        d.contact_force_scale, d.torque_scale = 0.01, 0.05
        rc = lib.lgx_bind_privileged_obs(h, C.c_void_p(buf.data_ptr()), C.byref(d))
        return rc, lib.lgx_last_error().decode()

    env.step(actions(0))
    for args, msg in (((47,), "below num_obs"), ((513,), "above LGX_MAX_PRIV_OBS"),
                      ((60, (6,), (48,)), "unknown term id"), ((60, (-1,), (48,)), "unknown term id"),
                      ((60, (5,), (47,)), "outside the tail"),          # into the clean part
                      ((60, (5,), (49,)), "outside the tail"),          # 49 + 12 > 60
                      ((80, (5, 0), (48, 59)), "terms overlap")):
        rc, err = bind(*args)
        assert rc == -1 and msg in err, (args, rc, err)
    assert lib.lgx_bind_privileged_obs(h, C.c_void_p(buf.data_ptr()), None) == -1
    # a refused bind leaves the bound row as it was
    _, row, *_ = env.step(actions(1))
    assert torch.equal(row, privileged_obs_ref(env))
    # unbind: the next steps write neither of the two old buffers
    old = [b.clone() for b in env._priv_bufs]
    bufs, env._priv_bufs = env._priv_bufs, None
    env._backend.bind_privileged_obs(None, None, 0.0, 0.0)
    assert lib.lgx_rebind_privileged_obs(h, C.c_void_p(buf.data_ptr())) == -1
    for k in (2, 3):
        env.step(actions(k))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, old))
    assert not buf.any()
    # and a valid bind of the clean part alone (terms == ()) writes exactly that
    rc, err = bind(48)
    assert rc == 0, err
    env.step(actions(4))
    want = privileged_obs_ref(env)[:, :48]
    assert torch.equal(buf.view(-1)[:N * 48].view(N, 48), want)
    assert not buf.view(-1)[N * 48:].any()


def test_go1_rough_asym_trains_end_to_end(gpu):
    """OnPolicyRunner.learn on go1_rough_asym: the critic's storage rows are the env's privileged
    rows, the rollout uses the fused act launch, the fused update runs with the two-input layer 1,
    and the critic's weights on the privileged columns move."""
    from legged_gym_amd.envs.go1.go1_config import Go1RoughCfgPPO
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    env = make_env("go1_rough_asym", num_envs=64, device="cuda:0", backend="lgx")
    assert env.num_privileged_obs == 253
    cfg = class_to_dict(Go1RoughCfgPPO())
    torch.manual_seed(0)
    runner = OnPolicyRunner(env, cfg, None, device="cuda:0")
    alg = runner.alg
    T = cfg["runner"]["num_steps_per_env"]
    assert alg._fused is not None and alg.actor_critic.critic[0].in_features == 253
    assert alg.actor_critic.actor[0].in_features == 235
    w0 = alg.actor_critic.critic[0].weight.detach().clone()
    rec = {"returned": [env.get_privileged_observations().clone()], "acted": [], "fused_act": [], "storage": [],
           "updates": 0, "separate": []}
    orig_act, orig_step, orig_update, orig_fused = alg.act, env.step, alg.update, alg._fused.update

    def act(obs, cobs):
        rec["acted"].append(cobs.clone())
        out = orig_act(obs, cobs)
        rec["fused_act"].append(alg.last_act_fused)
        return out

    def env_step(a):
        out = orig_step(a)
        rec["returned"].append(out[1].clone())
        return out

    def update(defer=False):
        rec["storage"].append(alg.storage.privileged_observations.clone())
        return orig_update(defer=defer)

    def fused_update(defer=False):
        rec["updates"] += 1
        rec["separate"].append(alg._fused._separate_critic_obs())
        return orig_fused(defer=defer)

    alg.act, env.step, alg.update, alg._fused.update = act, env_step, update, fused_update
    runner.learn(2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert len(rec["acted"]) == 2 * T and len(rec["storage"]) == 2
    assert all(rec["fused_act"]), "the rollout used the fused act launch"
    assert rec["updates"] == 2 and all(rec["separate"]), "FusedPPOUpdate ran with critic inputs of its own"
    for it in range(2):
        for s in range(T):
            k = it * T + s
            # the row the critic acted on at step k is the row the previous env.step returned ...
            assert torch.equal(rec["acted"][k], rec["returned"][k]), k
            # ... and it is what the storage holds for that step
            assert torch.equal(rec["storage"][it][s], rec["returned"][k]), k
            assert rec["returned"][k][:, 235:].any(), k
    fed = torch.stack([(st[..., 235:] != 0).flatten(0, 1).any(dim=0) for st in rec["storage"]]).any(dim=0)
    assert fed.all(), "every privileged column carried data in the rollouts"
    w1 = alg.actor_critic.critic[0].weight.detach()
    assert (w1[:, 235:] != w0[:, 235:]).any(dim=0).all(), "every privileged column's weights moved"
    for name, p in alg.actor_critic.named_parameters():
        assert torch.isfinite(p).all(), name


def test_train_script_runs_the_task_and_exports_the_actor_alone(gpu):
    """scripts/train.py --task go1_rough_asym trains and checkpoints; play.py resumes it and the
    exported policy is the actor: 235 observations in, no privileged input."""
    import os

    from legged_gym_amd import LEGGED_GYM_ROOT_DIR
    from legged_gym_amd.scripts.play import play
    from legged_gym_amd.scripts.train import train
    from legged_gym_amd.utils import get_args
    exp = f"pytest_asym_{os.getpid()}"
    common = ["--task", "go1_rough_asym", "--headless", "--num_envs", "64", "--experiment_name", exp]
    train(get_args(common + ["--max_iterations", "2"]))
    root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp)
    runs = os.listdir(root)
    assert len(runs) == 1 and "model_2.pt" in os.listdir(os.path.join(root, runs[0]))
    ck = torch.load(os.path.join(root, runs[0], "model_2.pt"), weights_only=True)["model_state_dict"]
    assert ck["critic.0.weight"].shape[1] == 253 and ck["actor.0.weight"].shape[1] == 235
    play(get_args(common + ["--load_run", runs[0]]), steps=20)
    pol = torch.jit.load(os.path.join(root, "exported", "policies", "policy_1.pt"))
    assert pol(torch.zeros(1, 235)).shape == (1, 12)
