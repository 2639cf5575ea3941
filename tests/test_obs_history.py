"""CPU: the observation history's layout, config surface, C-ABI declarations and the torch reference
model the GPU tests compare the kernel with (tests/obs_history_ref.py).  The reference project has
no observation history: the layout checked here is this project's own."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_arithmetic():
    from legged_gym_amd.envs.base.history import layout
    lay = layout(5, 48, 235)                  # go1_rough_hist
    assert lay.width == 475 and lay.obs == slice(0, 235) and lay.tail == slice(235, 475)
    assert [lay.frame(k) for k in (1, 2, 5)] == [slice(235, 283), slice(283, 331), slice(427, 475)]
    assert lay.source(1) == slice(0, 48) and lay.source(2) == lay.frame(1) and lay.source(5) == lay.frame(4)
    odd = layout(3, 45, 48)                   # frames that are no multiple of 4 wide
    assert odd.width == 183 and odd.frame(3) == slice(138, 183)
    assert layout(0, 48, 235) is None         # no history: no layout, whatever the frame width
    assert layout(0, 0, 235) is None
    assert layout(1, 48, 48).width == 96 and layout(1, 1, 48).width == 49
    assert layout(9, 48, 48).width == 480
    assert layout(29, 16, 48).width == 512    # the limit itself is allowed
    for k in (0, 6):
        with pytest.raises(ValueError, match="history of 5 frames"):
            lay.frame(k)


def test_layout_rejects_bad_configs():
    from legged_gym_amd.envs.base.history import layout
    with pytest.raises(ValueError, match="history.frames = -1"):
        layout(-1, 48, 235)
    with pytest.raises(ValueError, match=r"history.frame_width = 0.*\[1, num_observations = 48\]"):
        layout(2, 0, 48)
    with pytest.raises(ValueError, match="history.frame_width = 49"):
        layout(2, 49, 48)
    with pytest.raises(ValueError, match="row of 513 entries.*limit is 512"):
        layout(31, 15, 48)
    with pytest.raises(ValueError, match="limit is 512"):
        layout(6, 48, 235)                    # 523


def test_config_defaults_and_the_registered_task():
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.envs.base.history import layout
    from legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfg
    from legged_gym_amd.envs.go1.go1 import Go1
    from legged_gym_amd.envs.go1.go1_config import (Go1RoughAsymCfg, Go1RoughAsymHistCfg, Go1RoughCfgPPO,
                                                    Go1RoughTerrainCfg)
    from legged_gym_amd.utils.task_registry import task_registry
    d = LeggedRobotCfg()
    assert (d.history.frames, d.history.frame_width) == (0, 48)
    assert task_registry.get_task_class("go1_rough_hist") is Go1
    env_cfg, train_cfg = task_registry.get_cfgs("go1_rough_hist")
    assert isinstance(env_cfg, Go1RoughTerrainCfg) and isinstance(train_cfg, Go1RoughCfgPPO)
    assert (env_cfg.history.frames, env_cfg.history.frame_width) == (5, 48)
    assert env_cfg.env.num_privileged_obs is None and env_cfg.env.num_observations == 235
    # the pairing with the privileged critic is a config class, not a registered task
    both = Go1RoughAsymHistCfg()
    assert isinstance(both, Go1RoughAsymCfg) and (both.history.frames, both.history.frame_width) == (5, 48)
    assert both.env.num_privileged_obs == 253 and both.privileged.terms == Go1RoughAsymCfg().privileged.terms
    assert not any(isinstance(c, Go1RoughAsymHistCfg) for c in task_registry.env_cfgs.values())
    assert layout(env_cfg.history.frames, env_cfg.history.frame_width, env_cfg.env.num_observations).width == 475
    for name in task_registry.task_classes:       # every other task: no history
        if name != "go1_rough_hist":
            assert task_registry.get_cfgs(name)[0].history.frames == 0, name


def test_header_and_bindings_declare_the_entry_points():
    from legged_gym_amd.sim import abi
    txt = open(os.path.join(ROOT, "include", "lgx.h")).read()
    assert re.search(r"int lgx_bind_obs_history\(lgx_sim\* sim, float\* row, const float\* prev_row, "
                     r"const lgx_obs_history_desc\* desc\);", txt)
    assert re.search(r"int lgx_rebind_obs_history\(lgx_sim\* sim, float\* row, const float\* prev_row\);", txt)
    assert int(re.search(r"#define LGX_MAX_PRIV_OBS (\d+)", txt).group(1)) == abi.MAX_PRIV_OBS == 512


def test_library_exports_the_entry_points_and_checks_a_null_sim():
    """Host-side only: the null-sim check precedes any device call."""
    import torch  # noqa: F401  (HIP runtime first)
    from legged_gym_amd.sim import abi
    lib = abi.declare(C.CDLL(os.path.join(ROOT, "legged_gym_amd", "liblgx.so")))
    d = abi.LgxObsHistoryDesc(5, 48, 475)
    assert lib.lgx_bind_obs_history(None, C.c_void_p(0x1000), C.c_void_p(0x2000), C.byref(d)) == -1
    assert b"lgx_bind_obs_history: null sim" in lib.lgx_last_error()
    assert lib.lgx_bind_obs_history(None, None, None, None) == -1
    assert lib.lgx_rebind_obs_history(None, C.c_void_p(0x1000), C.c_void_p(0x2000)) == -1
    assert b"lgx_rebind_obs_history: null argument" in lib.lgx_last_error()


def test_no_history_builds_the_env_as_before_and_the_oracle_backend_refuses_one():
    from oracle_backend import make_env
    env = make_env("go1_flat_bench", num_envs=4)
    assert env.history_layout is None and env._hist_bufs is None
    assert env.num_obs == env.num_base_obs == 48 and env.obs_buf.shape == (4, 48)
    assert env.obs_buf is env._obs_bufs[env._obs_slot]
    obs = env.step(torch.zeros(4, 12))[0]
    assert obs.shape == (4, 48) and obs is env._obs_bufs[env._obs_slot]
    rough = make_env("go1_rough", num_envs=4)
    assert rough.num_obs == rough.num_base_obs == 235 and rough.noise_scale_vec.shape == (235,)

    def hist(frames, width=48):
        def override(cfg):
            cfg.history.frames, cfg.history.frame_width = frames, width
        return override
    with pytest.raises(ValueError, match="history.frames = 3: the backend OracleBackend cannot bind an observation "
                                         "history"):
        make_env("go1_flat_bench", num_envs=4, overrides=hist(3))
    with pytest.raises(ValueError, match="history.frames = -2"):
        make_env("go1_flat_bench", num_envs=4, overrides=hist(-2))
    with pytest.raises(ValueError, match="history.frame_width = 49"):
        make_env("go1_flat_bench", num_envs=4, overrides=hist(1, 49))
    with pytest.raises(ValueError, match="limit is 512"):
        make_env("go1_flat_bench", num_envs=4, overrides=hist(10))       # 48 + 480 = 528


# ---- the reference model on hand-made sequences: 1 env unless said, num_obs 3, W 2 (frames are
# the leading two entries), rows t = [10 t + 1, 10 t + 2, 10 t + 3]
def rows(n):
    return [torch.tensor([[10.0 * t + 1, 10.0 * t + 2, 10.0 * t + 3]]) for t in range(n)]


def run(ref, obs, resets, reset_idx_before=()):
    out = []
    for t, (o, r) in enumerate(zip(obs, resets)):
        if t in reset_idx_before:
            ref.reset_idx([0])
        out.append(ref.step(o, torch.tensor([r])))
    return out


def test_reference_reset_at_step_0_then_fills_one_frame_per_step():
    from obs_history_ref import ObsHistoryRef
    ref = ObsHistoryRef(1, 3, 3, 2)
    out = run(ref, rows(6), [True] + [False] * 5)
    want = [[1, 2, 3, 0, 0, 0, 0, 0, 0],
            [11, 12, 13, 1, 2, 0, 0, 0, 0],
            [21, 22, 23, 11, 12, 1, 2, 0, 0],
            [31, 32, 33, 21, 22, 11, 12, 1, 2],
            [41, 42, 43, 31, 32, 21, 22, 11, 12],       # a == H: the oldest frame drops out
            [51, 52, 53, 41, 42, 31, 32, 21, 22]]
    assert torch.equal(torch.cat(out), torch.tensor(want, dtype=torch.float32))
    assert ref.age.tolist() == [3] and ref.last_a.tolist() == [3]
    # without the reset at step 0 the result is the same: ages start at zero
    ref2 = ObsHistoryRef(1, 3, 3, 2)
    assert torch.equal(torch.cat(run(ref2, rows(6), [False] * 6)), torch.cat(out))


def test_reference_two_resets_closer_than_the_history():
    from obs_history_ref import ObsHistoryRef
    ref = ObsHistoryRef(1, 3, 3, 2)
    out = run(ref, rows(7), [False, False, True, False, True, False, False])
    want = [[1, 2, 3, 0, 0, 0, 0, 0, 0],
            [11, 12, 13, 1, 2, 0, 0, 0, 0],
            [21, 22, 23, 0, 0, 0, 0, 0, 0],             # reset in this step: the row has no past
            [31, 32, 33, 21, 22, 0, 0, 0, 0],           # ... and the rows before it never come back
            [41, 42, 43, 0, 0, 0, 0, 0, 0],             # second reset at a = 1 < H
            [51, 52, 53, 41, 42, 0, 0, 0, 0],
            [61, 62, 63, 51, 52, 41, 42, 0, 0]]
    assert torch.equal(torch.cat(out), torch.tensor(want, dtype=torch.float32))


def test_reference_reset_idx_between_steps_touches_one_env_only():
    from obs_history_ref import ObsHistoryRef
    ref = ObsHistoryRef(2, 3, 2, 2)
    two = lambda t: torch.tensor([[10.0 * t + 1, 10.0 * t + 2, 10.0 * t + 3], [-(10.0 * t + 1), -(10.0 * t + 2), 0.5]])
    no = torch.tensor([False, False])
    out = [ref.step(two(t), no) for t in range(3)]
    keep = out[-1].clone()
    ref.reset_idx([1])
    assert torch.equal(ref.prev, keep), "reset_idx touches no row"
    assert ref.age.tolist() == [2, 0]
    out.append(ref.step(two(3), no))
    assert out[3][0].tolist() == [31, 32, 33, 21, 22, 11, 12]          # env 0 goes on
    assert out[3][1].tolist() == [-31, -32, 0.5, 0, 0, 0, 0]           # env 1: its next tail is all zero
    out.append(ref.step(two(4), no))
    assert out[4][1].tolist() == [-41, -42, 0.5, -31, -32, 0, 0]
    # a reset_idx and an in-step reset of the same env in one step are one episode start
    ref.reset_idx([0])
    row = ref.step(two(5), torch.tensor([True, False]))
    assert row[0].tolist() == [51, 52, 53, 0, 0, 0, 0] and ref.age.tolist() == [1, 2]
