"""CPU: per-env actuator randomisation - the config surface, the function that draws the tables, the
C-ABI declarations and what needs no GPU of lgx_bind_actuator_rand.  The reference has no per-env
actuator: the semantics checked here and in tests/test_gpu_actuator_rand.py are this project's own."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("randomize_motor_strength", "randomize_kp", "randomize_kd", "randomize_lag")


def cfg_of(**kw):
    from legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfg
    c = types.SimpleNamespace(**{k: v for k, v in vars(LeggedRobotCfg.actuator_rand).items() if not k.startswith("_")})
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


ALL_ON = dict.fromkeys(FLAGS, True)


def test_config_defaults_are_off_and_domain_rand_is_the_reference_s():
    from legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfg
    a = LeggedRobotCfg().actuator_rand
    assert [getattr(a, f) for f in FLAGS] == [False] * 4
    assert a.motor_strength_range == [0.9, 1.1]
    assert a.kp_factor_range == [0.8, 1.2] and a.kd_factor_range == [0.8, 1.2]
    assert a.lag_substeps_range == [0, 4]
    names = {k for k in vars(LeggedRobotCfg.domain_rand) if not k.startswith("_")}
    assert names == {"randomize_friction", "friction_range", "randomize_base_mass", "added_mass_range",
                     "randomize_limb_mass", "added_limb_percentage", "push_robots", "push_interval_s", "max_push_vel_xy"}


def test_draw_all_off_gives_no_tables():
    from legged_gym_amd.envs.base.actuator_rand import draw
    assert draw(cfg_of(), 8, 12, 4, 1) == (None, None, None)
    assert draw(None, 8, 12, 4, 1) == (None, None, None)


def test_draw_shapes_dtypes_ranges_and_inclusive_lags():
    from legged_gym_amd.envs.base.actuator_rand import draw
    N = 4096
    kp, kd, lag = draw(cfg_of(**ALL_ON), N, 12, 4, 7)
    f = np.float32
    for t in (kp, kd):
        assert t.shape == (N, 12) and t.dtype == torch.float32 and t.is_contiguous()
        # strength in [0.9, 1.1] times a factor in [0.8, 1.2], one float32 product
        assert float(t.min()) >= float(f(0.9) * f(0.8)) and float(t.max()) <= float(f(1.1) * f(1.2))
        assert t.std() > 0.05 and (t[0] != t[1]).any() and (t[:, 0] != t[:, 1]).any()   # per env, per joint
    assert not torch.equal(kp, kd)
    assert lag.shape == (N,) and lag.dtype == torch.int32
    assert sorted(lag.unique().tolist()) == [0, 1, 2, 3, 4]          # both ends are drawn
    # one flag alone: only its table, inside its own range
    kp1, kd1, lag1 = draw(cfg_of(randomize_kp=True), N, 12, 4, 7)
    assert kd1 is None and lag1 is None
    assert float(kp1.min()) >= float(f(0.8)) and float(kp1.max()) <= float(f(1.2))
    # motor strength alone scales both gains by the same per-joint factor
    kp2, kd2, lag2 = draw(cfg_of(randomize_motor_strength=True), N, 12, 4, 7)
    assert torch.equal(kp2, kd2) and lag2 is None
    assert float(kp2.min()) >= float(f(0.9)) and float(kp2.max()) <= float(f(1.1))
    # the product of the two, in float32
    assert torch.equal(kp, draw(cfg_of(randomize_motor_strength=True, randomize_kp=True), N, 12, 4, 7)[0])
    strength, factor = kp2, kp1
    assert torch.equal(kp, strength * factor)
    _, _, lag3 = draw(cfg_of(randomize_lag=True, lag_substeps_range=[2, 2]), 16, 12, 4, 7)
    assert lag3.tolist() == [2] * 16


def test_draw_is_a_function_of_the_seed_and_leaves_the_global_streams_alone():
    from legged_gym_amd.envs.base.actuator_rand import draw
    a, b, c = draw(cfg_of(**ALL_ON), 64, 12, 4, 3), draw(cfg_of(**ALL_ON), 64, 12, 4, 3), draw(cfg_of(**ALL_ON), 64, 12, 4, 4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    torch.manual_seed(11)
    np.random.seed(11)
    t0, n0 = torch.rand(3), np.random.random_sample(3)
    torch.manual_seed(11)
    np.random.seed(11)
    draw(cfg_of(**ALL_ON), 64, 12, 4, 3)
    assert torch.equal(torch.rand(3), t0) and (np.random.random_sample(3) == n0).all()


def test_draw_rejects_bad_ranges():
    from legged_gym_amd.envs.base.actuator_rand import draw
    with pytest.raises(ValueError, match="kp_factor_range.*lower bound is above"):
        draw(cfg_of(randomize_kp=True, kp_factor_range=[1.2, 0.8]), 4, 12, 4, 1)
    with pytest.raises(ValueError, match="motor_strength_range.*must be > 0"):
        draw(cfg_of(randomize_motor_strength=True, motor_strength_range=[0.0, 1.0]), 4, 12, 4, 1)
    with pytest.raises(ValueError, match="kd_factor_range.*must be > 0"):
        draw(cfg_of(randomize_kd=True, kd_factor_range=[-0.5, 1.0]), 4, 12, 4, 1)
    with pytest.raises(ValueError, match="lag_substeps_range.*decimation = 4"):
        draw(cfg_of(randomize_lag=True, lag_substeps_range=[0, 5]), 4, 12, 4, 1)
    with pytest.raises(ValueError, match="lag_substeps_range"):
        draw(cfg_of(randomize_lag=True, lag_substeps_range=[-1, 2]), 4, 12, 4, 1)
    with pytest.raises(ValueError, match="lag_substeps_range.*lower bound is above"):
        draw(cfg_of(randomize_lag=True, lag_substeps_range=[3, 1]), 4, 12, 4, 1)
    # a range that is off is not looked at
    assert draw(cfg_of(randomize_kp=True, kd_factor_range=[2.0, 1.0]), 4, 12, 4, 1)[0] is not None


def test_header_and_bindings_declare_the_entry_point_and_the_struct():
    txt = open(os.path.join(ROOT, "include", "lgx.h")).read()
    assert re.search(r"int lgx_bind_actuator_rand\(lgx_sim\* sim, const lgx_actuator_rand_desc\* desc\);", txt)
    # no existing struct changed: the size table keeps its 12 entries
    assert re.search(r"void lgx_struct_sizes\(int64_t out\[12\]\);", txt)


def test_bind_validates_a_null_sim_without_a_gpu():
    """Host-side only: the null-sim check precedes any device call."""
    import torch  # noqa: F401  (HIP runtime first)
    from legged_gym_amd.sim import abi
    lib = abi.declare(C.CDLL(os.path.join(ROOT, "legged_gym_amd", "liblgx.so")))
    d = abi.LgxActuatorRandDesc(0x1000, None, None)
    assert lib.lgx_bind_actuator_rand(None, C.byref(d)) == -1
    assert b"lgx_bind_actuator_rand: null sim" in lib.lgx_last_error()
    assert lib.lgx_bind_actuator_rand(None, None) == -1


def test_oracle_backend_refuses_an_env_with_any_flag_set():
    """The CPU oracle has no per-env actuator: an env that asks for one on it fails at construction
    instead of silently simulating the nominal actuator."""
    from oracle_backend import make_env
    for flag in FLAGS:
        with pytest.raises(ValueError, match="OracleBackend cannot bind per-env actuator tables"):
            make_env("go1_flat_bench", num_envs=4, overrides=lambda cfg, f=flag: setattr(cfg.actuator_rand, f, True))

    def bad(cfg):
        cfg.actuator_rand.randomize_lag = True
        cfg.actuator_rand.lag_substeps_range = [0, 5]
    with pytest.raises(ValueError, match="lag_substeps_range"):
        make_env("go1_flat_bench", num_envs=4, overrides=bad)
    env = make_env("go1_flat_bench", num_envs=4)                      # the default: unchanged
    assert env.kp_scale is None and env.kd_scale is None and env.action_lag is None


def test_go1_rough_actrand_is_registered_and_every_other_task_is_off():
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.envs.go1.go1_config import Go1RoughCfgPPO, Go1RoughTerrainCfg
    from legged_gym_amd.utils.task_registry import task_registry
    assert task_registry.get_task_class("go1_rough_actrand") is Go1
    env_cfg, train_cfg = task_registry.get_cfgs("go1_rough_actrand")
    assert isinstance(env_cfg, Go1RoughTerrainCfg) and isinstance(train_cfg, Go1RoughCfgPPO)
    assert [getattr(env_cfg.actuator_rand, f) for f in FLAGS] == [True] * 4
    assert env_cfg.actuator_rand.lag_substeps_range[1] <= env_cfg.control.decimation
    assert env_cfg.env.num_observations == 235 and env_cfg.env.num_privileged_obs is None
    assert env_cfg.privileged.terms == () and env_cfg.history.frames == 0
    ref, _ = task_registry.get_cfgs("go1_rough")
    assert vars(type(env_cfg).domain_rand) == vars(type(ref).domain_rand) or all(
        getattr(env_cfg.domain_rand, k) == getattr(ref.domain_rand, k) for k in dir(ref.domain_rand) if not k.startswith("_"))
    for name in task_registry.task_classes:
        if name != "go1_rough_actrand":
            cfg, _ = task_registry.get_cfgs(name)
            assert [getattr(cfg.actuator_rand, f) for f in FLAGS] == [False] * 4, name
