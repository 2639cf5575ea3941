"""Task registrations (legged_gym/envs/__init__.py:52-59) for the robots in BASELINE scope.

go1 (configs C1/C2 defaults), go1_rough (C3/C4: trimesh + height scan), go1_rough_asym (go1_rough
with a privileged critic: env.num_privileged_obs + cfg.privileged), go1_rough_asym_norm (that task
with runner.empirical_normalization: running mean / std in front of actor and critic), go1_rough_hist (go1_rough with
an observation history: cfg.history), go1_rough_actrand (go1_rough with per-env drive gains and
action latency: cfg.actuator_rand), go1_rough_cmdcur (go1_rough with the command curriculum:
commands.curriculum, lin_vel_x widening from half of go1_rough's range), go1_rough_sym (go1_rough
trained with left-right symmetry data augmentation: algorithm.symmetry), go1_rough_mirror (go1_rough
trained with the symmetry mirror loss: algorithm.symmetry.use_mirror_loss), go1_rough_teacher
(go1_rough_asym with runner.privileged_actor: actor and critic read the privileged row),
go1_rough_distill (teacher-student distillation of such a teacher into a student on the 475-wide
history row: Distillation + StudentTeacher), go1_flat_bench (C2 as
BASELINE states it: PD, no domain randomisation), anymal_c_rough (C5), anymal_c_flat, and the
remaining robots of the reference registry: anymal_b, a1, a1_src, aliengo and cassie (the biped:
2 legs x 6 joints on the dense physics kernel).
"""
from legged_gym_amd import LEGGED_GYM_ENVS_DIR, LEGGED_GYM_ROOT_DIR  # noqa: F401
from legged_gym_amd.utils.task_registry import task_registry

from .a1.a1_config import A1RoughCfg, A1RoughCfgPPO, A1SrcRoughCfg, A1SrcRoughCfgPPO
from .aliengo.aliengo import Aliengo
from .aliengo.aliengo_config import AliengoRoughCfg, AliengoRoughCfgPPO
from .anymal_b.anymal_b_config import AnymalBRoughCfg, AnymalBRoughCfgPPO
from .anymal_c.anymal import Anymal
from .anymal_c.anymal_c_config import AnymalCFlatCfg, AnymalCFlatCfgPPO, AnymalCRoughCfg, AnymalCRoughCfgPPO
from .base.legged_robot import LeggedRobot
from .cassie.cassie import Cassie
from .cassie.cassie_config import CassieRoughCfg, CassieRoughCfgPPO
from .base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO
from .go1.go1 import Go1
from .go1.go1_config import (Go1FlatBenchCfg, Go1RoughActRandCfg, Go1RoughAsymCfg, Go1RoughAsymHistCfg, Go1RoughCfg,
                             Go1RoughCfgPPO, Go1RoughCmdCurCfg, Go1RoughDistillCfgPPO, Go1RoughHistCfg,
                             Go1RoughMirrorCfgPPO, Go1RoughNormCfgPPO, Go1RoughSymCfgPPO, Go1RoughSymMirrorCfgPPO,
                             Go1RoughTeacherCfgPPO, Go1RoughTerrainCfg)

task_registry.register("go1", Go1, Go1RoughCfg(), Go1RoughCfgPPO())
task_registry.register("go1_flat_bench", Go1, Go1FlatBenchCfg(), Go1RoughCfgPPO())
task_registry.register("go1_rough", Go1, Go1RoughTerrainCfg(), Go1RoughCfgPPO())
task_registry.register("go1_rough_asym", Go1, Go1RoughAsymCfg(), Go1RoughCfgPPO())
task_registry.register("go1_rough_hist", Go1, Go1RoughHistCfg(), Go1RoughCfgPPO())
task_registry.register("go1_rough_actrand", Go1, Go1RoughActRandCfg(), Go1RoughCfgPPO())
task_registry.register("anymal_c_rough", Anymal, AnymalCRoughCfg(), AnymalCRoughCfgPPO())
task_registry.register("anymal_c_flat", Anymal, AnymalCFlatCfg(), AnymalCFlatCfgPPO())
task_registry.register("anymal_b", Anymal, AnymalBRoughCfg(), AnymalBRoughCfgPPO())
task_registry.register("a1", LeggedRobot, A1RoughCfg(), A1RoughCfgPPO())
task_registry.register("a1_src", LeggedRobot, A1SrcRoughCfg(), A1SrcRoughCfgPPO())
task_registry.register("aliengo", Aliengo, AliengoRoughCfg(), AliengoRoughCfgPPO())
task_registry.register("cassie", Cassie, CassieRoughCfg(), CassieRoughCfgPPO())
# go1_rough_asym trained with runner.empirical_normalization: the same env, another train cfg
task_registry.register_variant("go1_rough_asym_norm", "go1_rough_asym", Go1RoughNormCfgPPO())
# go1_rough with commands.curriculum: the same env class, an env cfg of its own
task_registry.register_variant("go1_rough_cmdcur", "go1_rough", Go1RoughCfgPPO(), env_cfg=Go1RoughCmdCurCfg())
# go1_rough trained on its rollout rows and their mirror images: the same env, another train cfg
task_registry.register_variant("go1_rough_sym", "go1_rough", Go1RoughSymCfgPPO())
# go1_rough trained with the mirror loss on the actor's equivariance defect: the same env, another train cfg
task_registry.register_variant("go1_rough_mirror", "go1_rough", Go1RoughMirrorCfgPPO())
# go1_rough_asym with the privileged row as the actor's observations too: a teacher for go1_rough_distill
task_registry.register_variant("go1_rough_teacher", "go1_rough_asym", Go1RoughTeacherCfgPPO())
# the teacher distilled into a student that reads the observation history (475), the teacher the privileged row (253)
# (the same env class, Go1, with an env cfg of its own: a variant, so go1_rough_asym stays the one registered env
# with a privileged row and go1_rough_hist the one with a history)
task_registry.register_variant("go1_rough_distill", "go1_rough_asym", Go1RoughDistillCfgPPO(),
                               env_cfg=Go1RoughAsymHistCfg())
