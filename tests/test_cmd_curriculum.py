"""CPU: the command curriculum's rule (tests/cmd_curriculum_ref.py), the host's curriculum-step
predicate, the C-ABI of lgx_bind_command_curriculum / lgx_set_command_range, and the config
refusals that need no GPU.  The device side is tests/test_gpu_cmd_curriculum.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cmd_curriculum_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_lib():
    import torch  # noqa: F401  (HIP runtime first)
    from legged_gym_amd.sim import abi
    return abi.declare(C.CDLL(os.path.join(ROOT, "legged_gym_amd", "liblgx.so")))


def test_ref_clip_sequence():
    lo, hi = -0.3, 0.3
    seq = []
    for _ in range(3):
        lo, hi = ref.widen(lo, hi, 1.0)
        seq.append((lo, hi))
    assert seq == [(-0.8, 0.8), (-1.0, 1.0), (-1.0, 1.0)]
    # a start outside the clip interval behaves as np.clip does: pulled back to the bound, or to 0
    assert ref.widen(-2.0, 2.0, 1.0) == (-1.0, 1.0)
    assert ref.widen(0.7, -0.7, 1.0) == (0.0, 0.0)
    assert ref.widen(-0.5, 0.5, 0.0) == (0.0, 0.0)


def test_ref_decide_counts_only_moves_and_is_strict():
    L, scale = 8.0, 0.02
    thr = float(np.float32(0.8 * scale))
    on = dict(common_step_counter=16, max_episode_length=L, scale=scale, max_curriculum=1.0)
    assert ref.decide(-0.5, 0.5, 0, [thr * L * 1.25] * 3, **on)[:3] == (-1.0, 1.0, 1)
    assert ref.decide(-0.5, 0.5, 0, [thr * L * 0.75] * 3, **on)[:3] == (-0.5, 0.5, 0)
    assert ref.decide(-1.0, 1.0, 1, [thr * L * 1.25] * 3, **on)[:3] == (-1.0, 1.0, 1)      # clipped: no move
    assert ref.decide(-0.5, 0.5, 0, [thr * L] * 4, **on)[:3] == (-0.5, 0.5, 0)              # equal: not greater
    up = float(np.nextafter(np.float32(thr), np.float32(1)))
    assert ref.decide(-0.5, 0.5, 0, [up * L] * 4, **on)[:3] == (-1.0, 1.0, 1)
    assert ref.decide(-0.5, 0.5, 0, [], **on) == (-0.5, 0.5, 0, None)                       # no env reset
    assert ref.decide(-0.5, 0.5, 0, [1.0], **dict(on, common_step_counter=17)) == (-0.5, 0.5, 0, None)
    assert ref.decide(-0.5, 0.5, 0, [1.0], enabled=False, **on) == (-0.5, 0.5, 0, None)


def test_ref_draw_and_gate():
    cx, cy = ref.draw_xy([1.0, 0.5, 0.5625, 0.0], [1.0, 0.5, 0.5, 0.5], (-1.0, 1.0), (-1.0, 1.0))
    assert cx.tolist() == [1.0, 0.0, 0.0, -1.0] and cy.tolist() == [1.0, 0.0, 0.0, 0.0]    # 0.125 m/s is gated


@pytest.mark.parametrize("length", [8.0, 1001.0, np.float64(1001.0), np.ceil(20 / 0.02)])
def test_curriculum_step_predicate(length):
    """Host (Python) and library agree with `counter % max_episode_length == 0` for an integer-valued
    float length: counter 0, multiples, non-multiples."""
    from legged_gym_amd.envs.base.command_curriculum import is_curriculum_step
    lib = load_lib()
    n = int(length)
    for counter in (0, 1, n - 1, n, n + 1, 2 * n, 3 * n - 1, 7 * n, 7 * n + 3, 10 ** 9 * n, 10 ** 9 * n + 1):
        want = counter % length == 0
        assert want == (counter % n == 0)
        assert is_curriculum_step(counter, length) is bool(want), counter
        assert ref.is_curriculum_step(counter, length) == want
        assert lib.lgx_is_curriculum_step(counter, float(length)) == int(want), counter
    assert not is_curriculum_step(5, 0.0) and lib.lgx_is_curriculum_step(5, 0.0) == 0


def test_threshold_is_the_float64_product_as_float32():
    from legged_gym_amd.envs.base.command_curriculum import threshold
    scale = 1.0 * (4 * 0.005)
    assert threshold(scale).dtype == np.float32 and threshold(scale) == np.float32(0.8 * scale)


def test_desc_abi_matches_the_library_and_the_header():
    """The prototypes as written; the struct's layout and the entry points' argument classes are
    test_abi_host.py::test_bindings_mirror_the_header's, as for every other struct."""
    txt = open(os.path.join(ROOT, "include", "lgx.h")).read()
    assert re.search(r"int lgx_bind_command_curriculum\(lgx_sim\* sim, const lgx_cmd_curriculum_desc\* desc\);", txt)
    assert re.search(r"int lgx_set_command_range\(lgx_sim\* sim, int32_t k, float lo, float hi, void\* stream\);", txt)
    # no existing struct changed: the size table keeps its 12 entries
    assert re.search(r"void lgx_struct_sizes\(int64_t out\[12\]\);", txt)


def test_entry_points_validate_a_null_sim_without_a_gpu():
    from legged_gym_amd.sim import abi
    lib = load_lib()
    d = abi.LgxCmdCurriculumDesc(1.0, 0.016, 0x1000)
    assert lib.lgx_bind_command_curriculum(None, C.byref(d)) == -1
    assert b"lgx_bind_command_curriculum: null sim" in lib.lgx_last_error()
    assert lib.lgx_bind_command_curriculum(None, None) == -1
    assert lib.lgx_set_command_range(None, 0, -1.0, 1.0, None) == -1
    assert b"lgx_set_command_range: null sim" in lib.lgx_last_error()


def curriculum(extra=None):
    def override(cfg):
        cfg.commands.curriculum = True
        if extra:
            extra(cfg)
    return override


def test_oracle_backend_refuses_the_curriculum():
    """The CPU oracle backend has no binder: the switch raises instead of being dropped."""
    from oracle_backend import make_env
    with pytest.raises(ValueError, match="cannot bind a command curriculum"):
        make_env("go1", num_envs=4, device="cpu", backend="oracle", overrides=curriculum())
    env = make_env("go1", num_envs=4, device="cpu", backend="oracle")     # off: as before
    assert env.command_curriculum_state is None
    env.reset()
    assert "max_command_x" not in env.extras["episode"]


def test_config_refusals():
    from oracle_backend import make_env
    from legged_gym_amd.envs.base import command_curriculum as cc

    def no_tracking(cfg):
        cfg.rewards.scales.tracking_lin_vel = 0.0
    with pytest.raises(ValueError, match="tracking_lin_vel"):
        make_env("go1", num_envs=4, device="cpu", backend="oracle", overrides=curriculum(no_tracking))

    def negative_max(cfg):
        cfg.commands.max_curriculum = -1.0
    with pytest.raises(ValueError, match="max_curriculum"):
        make_env("go1", num_envs=4, device="cpu", backend="oracle", overrides=curriculum(negative_max))

    class Cmd:
        max_curriculum = 1.0
    nv = np.zeros(48)
    assert cc.validate(Cmd, {"tracking_lin_vel": 0.02}, nv) == (1.0, np.float32(0.8 * 0.02))
    with pytest.raises(ValueError, match="tracking_lin_vel"):
        cc.validate(Cmd, {"tracking_lin_vel": -0.02}, nv)
    with pytest.raises(ValueError, match="tracking_lin_vel"):
        cc.validate(Cmd, {}, nv)
    nv[10] = 0.1
    with pytest.raises(ValueError, match="noise_scale_vec"):
        cc.validate(Cmd, {"tracking_lin_vel": 0.02}, nv)


def test_set_command_range_updates_the_host_copies():
    """Without a device range (the oracle backend reads the host params on every call) the setter
    still updates env.command_ranges and the params struct."""
    from oracle_backend import make_env
    env = make_env("go1", num_envs=4, device="cpu", backend="oracle")
    env.set_command_range("lin_vel_y", -0.25, 0.75)
    assert env.command_ranges["lin_vel_y"] == [-0.25, 0.75]
    assert list(env._lgx_params.cmd_ranges[1]) == [-0.25, 0.75]
    assert env.sync_command_ranges() is env.command_ranges
    with pytest.raises(ValueError):
        env.set_command_range("lin_vel_z", 0.0, 1.0)


def test_cmdcur_task_is_a_variant_of_go1_rough():
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.utils.task_registry import task_registry
    cur, _ = task_registry.get_cfgs("go1_rough_cmdcur")
    base, _ = task_registry.get_cfgs("go1_rough")
    assert task_registry.get_task_class("go1_rough_cmdcur") is Go1
    assert "go1_rough_cmdcur" not in task_registry.task_classes and "go1_rough_cmdcur" not in task_registry.env_cfgs
    assert cur is not base and cur.commands.curriculum is True and base.commands.curriculum is False
    b = base.commands.ranges.lin_vel_x
    assert cur.commands.ranges.lin_vel_x == [0.5 * b[0], 0.5 * b[1]]
    assert cur.commands.max_curriculum == b[1] == -b[0]
    assert cur.commands.ranges.lin_vel_y == base.commands.ranges.lin_vel_y
    assert cur.env.num_observations == base.env.num_observations and cur.env.num_privileged_obs is None
