"""Go1 task configs (reference: legged_gym/envs/go1/go1_config.py:34-110).

`Go1RoughCfg` is the reference's Go1 config (despite the name: flat `plane`, 48-dim obs).
`Go1RoughTerrainCfg` is BASELINE config C3/C4: the same robot on the curriculum trimesh
with the 187-point height scan (235-dim obs), as SURVEY.md §8 defines it.
`Go1RoughAsymCfg` is that task with an asymmetric actor-critic: the critic reads the privileged
row (noise-free observations + the randomised friction / base mass + foot contacts).
`Go1RoughHistCfg` is go1_rough with an observation history, registered as
go1_rough_hist; `Go1RoughAsymHistCfg` pairs the history with the privileged critic (the env of the
go1_rough_distill variant; not a registered env of its own).
`Go1RoughActRandCfg` is go1_rough with per-env drive gains and action latency,
registered as go1_rough_actrand.
`Go1RoughCmdCurCfg` is go1_rough with the command curriculum, registered as
go1_rough_cmdcur.
`Go1RoughSymCfgPPO` trains with left-right symmetry data augmentation: go1_rough under
it is registered as go1_rough_sym; `Go1RoughAsymHistSymCfg` names the widest combination (history actor,
privileged critic) meant to be trained with it (not registered).
`Go1RoughMirrorCfgPPO` trains with the symmetry mirror loss alone: go1_rough under it is
registered as go1_rough_mirror; `Go1RoughSymMirrorCfgPPO` pairs the mirror loss with the augmentation (not
registered).
`Go1RoughTeacherCfgPPO` trains a privileged teacher (runner.privileged_actor; go1_rough_asym under it is
go1_rough_teacher) and `Go1RoughDistillCfgPPO` distils it into a student on the history row
(Go1RoughAsymHistCfg under it is go1_rough_distill).
"""
from legged_gym_amd.envs.base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO


class Go1RoughCfg(LeggedRobotCfg):
    class env(LeggedRobotCfg.env):
        num_observations = 48

    class terrain(LeggedRobotCfg.terrain):
        mesh_type = 'plane'
        measure_heights = False

    class init_state(LeggedRobotCfg.init_state):
        pos = [0.0, 0.0, 0.32]
        default_joint_angles = {   # target angles [rad] for action = 0
            'FL_hip_joint': 0.1, 'RL_hip_joint': 0.1, 'FR_hip_joint': -0.1, 'RR_hip_joint': -0.1,
            'FL_thigh_joint': 0.8, 'RL_thigh_joint': 1., 'FR_thigh_joint': 0.8, 'RR_thigh_joint': 1.,
            'FL_calf_joint': -1.5, 'RL_calf_joint': -1.5, 'FR_calf_joint': -1.5, 'RR_calf_joint': -1.5,
        }

    class control(LeggedRobotCfg.control):
        control_type = 'P'
        stiffness = {'hip_joint': 30, 'thigh_joint': 50., 'calf_joint': 50.}
        damping = {'hip_joint': 2., 'thigh_joint': 2., 'calf_joint': 2.}
        action_scale = 0.25
        decimation = 4
        use_actuator_network = True
        actuator_net_file = "{LEGGED_GYM_ROOT_DIR}/resources/actuator_nets/go1_net.npz"

    class asset(LeggedRobotCfg.asset):
        file = '{LEGGED_GYM_ROOT_DIR}/resources/go1_model.json'
        name = "go1"
        foot_name = "foot"
        penalize_contacts_on = ["thigh", "calf"]
        terminate_after_contacts_on = ["base"]
        self_collisions = 1

    class domain_rand(LeggedRobotCfg.domain_rand):
        randomize_base_mass = True
        added_mass_range = [-1., 1.]
        randomize_limb_mass = True
        added_limb_percentage = [-0.2, 0.2]

    class rewards(LeggedRobotCfg.rewards):
        soft_dof_pos_limit = 0.9
        base_height_target = 0.25

        class scales(LeggedRobotCfg.rewards.scales):
            torques = -0.00025
            dof_pos_limits = -10.0


class Go1RoughCfgPPO(LeggedRobotCfgPPO):
    class algorithm(LeggedRobotCfgPPO.algorithm):
        entropy_coef = 0.01

    class runner(LeggedRobotCfgPPO.runner):
        run_name = ''
        experiment_name = 'rough_go1'


class Go1RoughNormCfgPPO(Go1RoughCfgPPO):
    """Go1RoughCfgPPO with empirical observation normalisation in front of the actor and the critic."""
    class runner(Go1RoughCfgPPO.runner):
        empirical_normalization = True


class Go1RoughSymCfgPPO(Go1RoughCfgPPO):
    """Go1RoughCfgPPO with symmetry data augmentation: every minibatch holds its rollout rows and
    their mirror images (rsl_rl 2.x symmetry_cfg.use_data_augmentation)."""
    class algorithm(Go1RoughCfgPPO.algorithm):
        class symmetry(Go1RoughCfgPPO.algorithm.symmetry):
            use_data_augmentation = True


class Go1RoughMirrorCfgPPO(Go1RoughCfgPPO):
    """Go1RoughCfgPPO with the symmetry mirror loss alone (rsl_rl 2.x symmetry_cfg.use_mirror_loss without
    use_data_augmentation): the PPO terms run over the rollout rows as in go1_rough, and
    mirror_loss_coeff x mean((mu(mirror(o)) - mirror(mu(o)))^2) penalises the actor's equivariance
    defect on every minibatch.  The update costs what go1_rough_sym's does (the actor and the critic
    run over the mirror rows too).  mirror_loss_coeff = 1.0 is untuned: no learning curve has been
    produced with it."""
    class algorithm(Go1RoughCfgPPO.algorithm):
        class symmetry(Go1RoughCfgPPO.algorithm.symmetry):
            use_mirror_loss = True
            mirror_loss_coeff = 1.0


class Go1RoughSymMirrorCfgPPO(Go1RoughCfgPPO):
    """Go1RoughSymCfgPPO plus the mirror loss (both halves of rsl_rl 2.x symmetry_cfg): the PPO terms
    over the rollout rows and their mirror images, the mirror term on top.  mirror_loss_coeff is
    untuned, as in Go1RoughMirrorCfgPPO."""
    class algorithm(Go1RoughCfgPPO.algorithm):
        class symmetry(Go1RoughSymCfgPPO.algorithm.symmetry):
            use_mirror_loss = True
            mirror_loss_coeff = 1.0


class Go1FlatBenchCfg(Go1RoughCfg):
    """BASELINE config C2: flat, PD actuator, no domain randomisation."""
    class control(Go1RoughCfg.control):
        use_actuator_network = False

    class domain_rand(Go1RoughCfg.domain_rand):
        randomize_friction = False
        randomize_base_mass = False
        randomize_limb_mass = False
        push_robots = False


class Go1RoughTerrainCfg(Go1RoughCfg):
    """BASELINE config C3/C4: curriculum trimesh + 187-point height scan, actuator net on."""
    class env(Go1RoughCfg.env):
        num_observations = 235

    class terrain(Go1RoughCfg.terrain):
        mesh_type = 'trimesh'
        measure_heights = True


class Go1RoughAsymCfg(Go1RoughTerrainCfg):
    """go1_rough with a privileged critic (no reference counterpart): the actor sees the noisy 235
    observations, the critic the same 235 before noise plus friction, base mass scale, foot contact
    flags and scaled foot contact forces (1 + 1 + 4 + 12 = 18)."""
    class env(Go1RoughTerrainCfg.env):
        num_privileged_obs = 253

    class privileged(Go1RoughTerrainCfg.privileged):
        terms = ("friction", "base_mass", "feet_contact", "feet_forces")

    class domain_rand(Go1RoughTerrainCfg.domain_rand):
        randomize_friction = True
        randomize_base_mass = True


class Go1RoughHistCfg(Go1RoughTerrainCfg):
    """go1_rough with a proprioceptive history (no reference counterpart): the observation row is the
    noisy 235 observations plus the leading 48 entries of the last 5 rows (235 + 5 * 48 = 475,
    envs/base/history.py).  No privileged row: the critic reads the same 475 entries."""
    class history(Go1RoughTerrainCfg.history):
        frames = 5


class Go1RoughActRandCfg(Go1RoughTerrainCfg):
    """go1_rough with the actuator randomised per env (no reference counterpart): motor strength, PD
    gains and an action latency of 0 .. 4 substeps (envs/base/actuator_rand.py).  No privileged row and
    no history: the policy has to be robust to what it cannot observe."""
    class actuator_rand(Go1RoughTerrainCfg.actuator_rand):
        randomize_motor_strength = True
        randomize_kp = True
        randomize_kd = True
        randomize_lag = True


class Go1RoughCmdCurCfg(Go1RoughTerrainCfg):
    """go1_rough with the reference's command curriculum (commands.curriculum, legged_robot.py:465-474):
    lin_vel_x starts half as wide as go1_rough's and widens by 0.5 m/s per bound, up to go1_rough's
    range, whenever the envs that reset on a curriculum step tracked their velocity command well."""
    class commands(Go1RoughTerrainCfg.commands):
        curriculum = True
        max_curriculum = Go1RoughTerrainCfg.commands.ranges.lin_vel_x[1]

        class ranges(Go1RoughTerrainCfg.commands.ranges):
            lin_vel_x = [0.5 * v for v in Go1RoughTerrainCfg.commands.ranges.lin_vel_x]


class Go1RoughAsymHistCfg(Go1RoughAsymCfg):
    """go1_rough_asym with that history for the actor: actor 475 wide, critic the 253-wide privileged
    row.  Not a registered env (go1_rough_asym is the one registered env with a privileged row; the
    go1_rough_distill variant trains on this cfg); to train PPO on it register it under a name of
    your own: task_registry.register(name, Go1, Go1RoughAsymHistCfg(), Go1RoughCfgPPO())."""
    class history(Go1RoughAsymCfg.history):
        frames = 5


class Go1RoughAsymHistSymCfg(Go1RoughAsymHistCfg):
    """go1_rough with the 475-wide history row for the actor and the 253-wide privileged row for the
    critic, to be trained under Go1RoughSymCfgPPO: all three mirror tables (history frames, privileged
    tail, actions) are in use.  Not in the registry: task_registry.register(name, Go1,
    Go1RoughAsymHistSymCfg(), Go1RoughSymCfgPPO())."""


class Go1RoughTeacherCfgPPO(Go1RoughCfgPPO):
    """Go1RoughCfgPPO training a privileged teacher: the env's privileged row is the
    one observation row of actor and critic.  go1_rough_asym under it is registered as
    go1_rough_teacher; its checkpoints are what go1_rough_distill loads."""
    class runner(Go1RoughCfgPPO.runner):
        privileged_actor = True
        experiment_name = 'rough_go1_teacher'


class Go1RoughDistillCfgPPO(LeggedRobotCfgPPO):
    """Teacher-student distillation (rsl_rl 2.x Distillation + StudentTeacher): the
    student reads the 475-wide history row of Go1RoughAsymHistCfg, the teacher - a go1_rough_teacher
    checkpoint's actor - the 253-wide privileged row.  Registered as go1_rough_distill:
        --task go1_rough_distill --resume --load_run <a go1_rough_teacher run>
    (both tasks log under rough_go1_teacher, so --load_run finds the teacher's run).  Every value
    below is untuned: no distilled student has been evaluated."""
    class policy:
        init_noise_std = 0.1
        student_hidden_dims = [512, 256, 128]
        teacher_hidden_dims = [512, 256, 128]   # the teacher run's actor_hidden_dims
        activation = 'elu'

    class algorithm:
        num_learning_epochs = 1
        gradient_length = 12
        learning_rate = 1.e-3
        max_grad_norm = None
        loss_type = 'mse'

    class runner(LeggedRobotCfgPPO.runner):
        policy_class_name = 'StudentTeacher'
        algorithm_class_name = 'Distillation'
        num_steps_per_env = 24
        run_name = ''
        experiment_name = 'rough_go1_teacher'
