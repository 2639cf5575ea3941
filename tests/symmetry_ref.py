"""Shared by tests/test_symmetry.py and tests/test_gpu_symmetry.py: the mirror tables of a registered
task built from its config alone (no env: the CPU oracle backend binds neither a privileged row nor a
history), the numpy statement of the augment launch, and the reflected-state construction of the
physical check of the signs."""
import numpy as np
import torch

import legged_gym_amd.envs  # noqa: F401  (registrations)
from legged_gym_amd import LEGGED_GYM_ROOT_DIR
from legged_gym_amd.envs.base import history, privileged, symmetry
from legged_gym_amd.sim.model import RobotAsset, resolve_asset_path

# tests/test_gpu_parity.py docstring: multi-step float32 comparisons
VEL_ATOL, VEL_RTOL, POS_ATOL = 2e-3, 2e-3, 1e-4
VEL_COLS = list(range(0, 6)) + list(range(24, 36))      # base lin / ang velocity, dof velocities


def cfg_tables(cfg):
    """symmetry.env_tables of an env config (lists), as LeggedRobot.symmetry_tables builds them."""
    asset = RobotAsset(resolve_asset_path(cfg.asset.file, LEGGED_GYM_ROOT_DIR))
    feet = [n for n in asset.body_names if cfg.asset.foot_name in n]
    num_obs = cfg.env.num_observations
    q0 = [cfg.init_state.default_joint_angles[n] for n in asset.dof_names]
    priv = None
    if cfg.env.num_privileged_obs is not None:
        priv = privileged.layout(cfg.privileged.terms, num_obs, len(feet), cfg.env.num_privileged_obs)
    hist = history.layout(cfg.history.frames, cfg.history.frame_width, num_obs)
    measure = cfg.terrain.measure_heights
    return symmetry.env_tables(asset.data, asset.dof_names, [b["name"] for b in asset.data["dyn_bodies"]], feet, q0,
                               num_obs, cfg.terrain.measured_points_x if measure else (),
                               cfg.terrain.measured_points_y if measure else (), priv, hist)


def as_tensors(tables, device="cpu"):
    return {k: None if v is None else (torch.tensor(v[0], dtype=torch.int32, device=device),
                                       torch.tensor(v[1], dtype=torch.float32, device=device))
            for k, v in tables.items()}


def mirror(x, table):
    """torch mirroring through a (perm int32, sign float32) table."""
    return symmetry.apply(x, table[0].long(), table[1])


def augment_numpy(arrays, tables, B):
    """What lgx_ppo_symmetry_augment writes to rows [B, 2B) of every array from rows [0, B):
    {name: the expected [B, ...] block} (numpy, exact: a copy and a sign flip)."""
    t = {k: None if v is None else (np.asarray(v[0]), np.asarray(v[1], dtype=np.float32)) for k, v in tables.items()}
    out = {}
    for name, a in arrays.items():
        real = a[:B]
        if name == "observations":
            out[name] = real[:, t["obs"][0]] * t["obs"][1]
        elif name == "privileged_observations":
            out[name] = real[:, t["critic_obs"][0]] * t["critic_obs"][1]
        elif name in ("actions", "mu"):
            out[name] = real[:, t["actions"][0]] * t["actions"][1]
        elif name == "sigma":
            out[name] = real[:, t["actions"][0]]
        else:
            out[name] = real.copy()
    return out


def no_noise(cfg):
    cfg.noise.add_noise = False
    cfg.domain_rand.push_robots = False
    cfg.domain_rand.randomize_friction = False


class mirror_symmetric_model:
    """Context: robot models loaded inside have exactly mirror-symmetric inertial data (each right
    body's centre of mass and inertia tensor = its left partner's reflected; the base's centre of mass
    on the x-z plane, its xy / yz products of inertia zero).  The committed Go1 model is the URDF's: its
    base centre of mass lies 2.0 mm off the plane and the left / right calf centres differ by 1.8 mm
    in y, so its dynamics commute with the mirror only to that level (measured: 6.0e-3 on the scaled
    base velocity columns, 1.9e-4 on the position columns after one step of smooth_state) - above the
    float32 bounds the physical check of the signs uses, which presuppose a symmetric robot."""

    def __enter__(self):
        import legged_gym_amd.envs.base.legged_robot as lr
        self.lr, self.orig = lr, lr.RobotAsset

        class Symmetric(lr.RobotAsset):
            def __init__(asset, path):
                super().__init__(path)
                bodies = asset.data["dyn_bodies"]
                names = [b["name"] for b in bodies]
                twin = symmetry.partners(names, symmetry.leg_pairs(asset.dof_names))
                base = bodies[0]
                base["com"][1] = base["inertia"][3] = base["inertia"][5] = 0.0
                for i, j in enumerate(twin):
                    if j > i:     # inertia: xx, yy, zz, xy, xz, yz
                        c, I = bodies[i]["com"], bodies[i]["inertia"]
                        bodies[j]["com"] = [c[0], -c[1], c[2]]
                        bodies[j]["inertia"] = [I[0], I[1], I[2], -I[3], I[4], -I[5]]
                        bodies[j]["mass"] = bodies[i]["mass"]
        lr.RobotAsset = Symmetric
        return self

    def __exit__(self, *exc):
        self.lr.RobotAsset = self.orig
        return False


def smooth_state(env, gen):
    """A state of test_gpu_parity.randomize_state made smooth for one env step: the base 1 m above the
    plane (no contact), joint offsets, velocities and actions small enough that no joint limit or
    torque saturation is reached, no command resampling or time-out in the step; every hip offset
    (>= 0.1 rad), hip velocity (>= 1 rad/s), base vy (>= 0.25 m/s) and yaw rate (>= 0.4 rad/s) away
    from zero, so a missing sign shows.  Returns the actions to step with."""
    from test_gpu_parity import randomize_state
    randomize_state(env, gen)
    N = env.num_envs
    r = lambda *s: torch.rand(*s, generator=gen)
    pm = lambda *s: torch.where(r(*s) < 0.5, -1.0, 1.0)
    hips = [j for j, n in enumerate(env.dof_names) if "hip" in n or "HAA" in n]
    env.root_states[:, 2] += 1.0
    off = (r(N, 12) - 0.5) * 0.3
    off[:, hips] = pm(N, len(hips)) * (0.1 + 0.1 * r(N, len(hips)))
    env.dof_pos[:] = env.default_dof_pos + off
    vel = (r(N, 12) - 0.5) * 2.0
    vel[:, hips] = pm(N, len(hips)) * (1.0 + r(N, len(hips)))
    env.dof_vel[:] = vel
    env.root_states[:, 8] = pm(N) * (0.25 + 0.25 * r(N))      # world vy
    env.root_states[:, 12] = pm(N) * (0.4 + 0.4 * r(N))       # world yaw rate
    env.actions[:] = (r(N, 12) - 0.5) * 0.6
    env.target_poses[:] = env.actions * env.cfg.control.action_scale + env.default_dof_pos
    env._episode_length_buf[:] = 5
    return (r(N, 12) - 0.5) * 0.6


def mirrored_envs(device="cpu", backend="oracle", num_envs=16):
    """Two go1_flat_bench envs (no noise, pushes or friction randomisation) on the mirror-symmetric model."""
    from oracle_backend import make_env
    with mirror_symmetric_model():
        return [make_env("go1_flat_bench", num_envs=num_envs, device=device, backend=backend, overrides=no_noise)
                for _ in range(2)]


def reflect_state(src, dst, tables):
    """dst's state = src's reflected across the world x-z plane: root y negated, quaternion
    (x, y, z, w) -> (-x, y, -z, w), linear velocity (+, -, +), angular velocity (-, +, -), joint
    quantities through the action table, commands (+, -, -) and the heading command negated."""
    act = tables["actions"]
    m = lambda x: mirror(x, act)
    rs = src.root_states.clone()
    rs[:, 1] = -rs[:, 1]
    rs[:, 3] = -rs[:, 3]
    rs[:, 5] = -rs[:, 5]
    rs[:, 8] = -rs[:, 8]
    rs[:, 10] = -rs[:, 10]
    rs[:, 12] = -rs[:, 12]
    dst.root_states.copy_(rs)
    dst.dof_pos[:] = m(src.dof_pos)
    dst.dof_vel[:] = m(src.dof_vel)
    for name in ("actions", "last_actions", "last_dof_vel", "target_poses"):
        getattr(dst, name).copy_(m(getattr(src, name)))
    dst.commands.copy_(src.commands * torch.tensor([1.0, -1.0, -1.0, -1.0]))
    dst._episode_length_buf.copy_(src._episode_length_buf)


def assert_smooth(env):
    """No joint limit and no torque saturation after the step (the last substep's torques)."""
    lim = env.torque_limits
    assert (env.torques.abs() <= 0.9 * lim).all(), (env.torques.abs() / lim).max().item()
    lo, hi = env.dof_pos_limits[:, 0], env.dof_pos_limits[:, 1]
    assert ((env.dof_pos > lo) & (env.dof_pos < hi)).all()
    assert not env.reset_buf.any()


def assert_pd_unsaturated(env, actions):
    """The PD torque the drive asks for at the start state stays below the limit too."""
    target = actions * env.cfg.control.action_scale + env.default_dof_pos
    tau = env.p_gains * (target - env.dof_pos) - env.d_gains * env.dof_vel
    assert (tau.abs() <= 0.9 * env.torque_limits).all(), (tau.abs() / env.torque_limits).max().item()


def obs_bound(ref):
    """|d| <= 2e-3 + 2e-3 |x| on the velocity columns, 1e-4 on the others (per element of ref)."""
    b = torch.full_like(ref, POS_ATOL)
    b[:, VEL_COLS] = VEL_ATOL + VEL_RTOL * ref[:, VEL_COLS].abs()
    return b


def assert_obs_close(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    err, bound = (got - ref).abs(), obs_bound(ref)
    print(f"{what}: max |d| velocity columns {err[:, VEL_COLS].max().item():.3e}, other columns "
          f"{err[:, [c for c in range(ref.shape[1]) if c not in VEL_COLS]].max().item():.3e}")
    assert (err <= bound).all(), (what, (err - bound).max().item(), (err > bound).nonzero()[:8].tolist())
