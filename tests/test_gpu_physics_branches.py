"""GPU: every physics kernel formulation on the branch states of tests/physics_branch_states.py -
joints outside and crossing their limits, the joint velocity clamp, saturated drives of every joint
and sign, a limit under contact load - 64 envs, 4 substeps, HIP against the float64 oracle with the
derived tolerance of test_gpu_parity.check_derived (constants unchanged).

What the states reach is asserted on the float64 records by the CPU test
(tests/test_physics_branches.py), which also holds every constructed decision away from its
threshold; here each case additionally requires that no outlier had to be explained by flipping a
drive or limit decision of a constructed row's constructed joint (BRANCH_FLIPS).  The CPU reference
of a (task, class) is computed once per session and shared by the cases.

Run with -s for the worst-env ratio of HIP's error to the float32 oracle's, per class."""
import pytest
import torch

import physics_branch_states as S
import test_gpu_parity as P
from oracle_backend import make_env
from test_gpu_parity import PHYS_QTY, check_derived, close, sync

pytestmark = pytest.mark.gpu

N, NSUB = S.N, S.NSUB


def device_env(task, overrides=None):
    return make_env(task, num_envs=N, device="cuda:0", backend="lgx", overrides=overrides)


def simulate_from(ref, dev):
    """`dev` from the reference's start state, NSUB substeps; its physics quantities on the host."""
    S.load_start(ref)
    sync(ref.ora, dev)
    if hasattr(ref.ora, "terrain_types"):
        dev.terrain_types.copy_(ref.ora.terrain_types)
    dev.simulate(NSUB)
    torch.cuda.synchronize()
    return {k: f(dev).detach().cpu().clone() for k, f in PHYS_QTY.items()}


def no_constructed_flip(ref, flips):
    """No explained outlier of this comparison flipped a drive / limit decision of a constructed joint."""
    for f in flips:
        j = int(ref.plan.joint[f["env"]])
        bad = [d for d in f["flips"] if d[0] in ("drive", "limit") and d[2] == f"index {j}"]
        assert not bad, f"class {ref.cls} env {f['env']}: the constructed joint {j} needed a branch flip: {f}"


def compare(ref, hip, label, keep=None):
    """check_derived on every quantity, no flip of a constructed decision, class G's contact forces
    on their own; prints and returns the worst-env ratios HIP error / float32-oracle error."""
    n0 = len(P.BRANCH_FLIPS)
    for k, v in hip.items():
        assert torch.isfinite(v).all(), (label, ref.cls, k)
    errs = check_derived(ref.t64, ref.o32, hip, keep=keep)
    if ref.cls == "G":
        rows = ref.plan.joint >= 0
        if keep is not None:
            rows = rows & keep
        touching = ref.t64["contact_forces"].abs().amax((1, 2)) > 0
        assert (rows & touching).sum() >= 4, "class G rows should carry contact forces"
        check_derived(ref.t64, ref.o32, hip, keep=rows & touching, qty=["contact_forces"])
        assert (hip["contact_forces"][rows & touching].abs().amax((1, 2)) > 0).all()
    no_constructed_flip(ref, P.BRANCH_FLIPS[n0:])
    ratios = {k: h / o if o > 0 else float("nan") for k, (h, o) in errs.items()}
    print(f"{label:24s} {ref.cls}: " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items())
          + f"  flips {len(P.BRANCH_FLIPS) - n0}")
    return ratios


def run_classes(task, dev, label, classes=S.CLASSES):
    out = {}
    for cls in classes:
        ref = S.reference(task, cls)
        out[cls] = simulate_from(ref, dev)
        compare(ref, out[cls], label)
    return out


@pytest.mark.parametrize("task", ["go1_flat_bench", "go1_rough", "aliengo"])
def test_arrowhead_kernel_on_branch_states(gpu, task):
    """lgx_physics_kernel at the default lane split; Aliengo's first comparison at the derived tolerance."""
    dev = device_env(task)
    assert dev._lgx_model.leg_dof != 6
    run_classes(task, dev, task)


def test_limits_that_differ_by_leg(gpu):
    """Go1 loaded with limits shifted leg by leg (physics_branch_states.per_leg_limits): the limit
    classes on the arrowhead kernel, whose joint 3 leg + k must read its own leg's limits."""
    task = "go1_flat_bench"
    with S.per_leg_limits():
        dev = device_env(task)
    lo = [dev._lgx_model.dof_lower[j] for j in range(12)]
    assert len(set(lo)) == 12
    for cls in "ABCEG":
        ref = S.legs_reference(task, cls)
        compare(ref, simulate_from(ref, dev), task + " per-leg limits")


@pytest.mark.parametrize("pp", ["1", "2", "8"])
def test_every_lane_split_on_branch_states(gpu, monkeypatch, pp):
    monkeypatch.setenv("LGX_PHYS_PP", pp)
    run_classes("go1_flat_bench", device_env("go1_flat_bench"), f"go1_flat_bench pp={pp}")


def test_dense_kernel_on_branch_states(gpu, monkeypatch):
    """lgx_physics_dense_kernel on the quadruped (LGX_PHYS_DENSE=1) against float64, and the arrowhead
    kernel from the same states: two formulations, one truth."""
    arrow = device_env("go1_flat_bench")
    monkeypatch.setenv("LGX_PHYS_DENSE", "1")
    dense = device_env("go1_flat_bench")
    d = run_classes("go1_flat_bench", dense, "go1_flat_bench dense")
    a = run_classes("go1_flat_bench", arrow, "go1_flat_bench arrowhead")
    assert any(not torch.equal(d[c]["dof_vel"], a[c]["dof_vel"]) for c in S.CLASSES), "LGX_PHYS_DENSE=1 selected no other kernel"


def test_cassie_dense_kernel_on_branch_states(gpu):
    """The dense kernel at leg_dof == 6: limits, clamp and saturation (efforts 112, 195, 45 N m) of all 12 joints."""
    dev = device_env("cassie")
    assert dev._lgx_model.leg_dof == 6
    run_classes("cassie", dev, "cassie")


def test_per_env_gains_on_branch_states(gpu):
    """The lgx_physics_rand.hip instantiation with gains that differ per env (bound as
    tests/test_gpu_actuator_rand.py binds them): saturation thresholds and the implicit drive's Dimp
    differ per row.  Each gain table's envs against the float64 run of a model with those gains."""
    task = "go1_flat_bench"
    dev = device_env(task)
    ora = S.oracle_env(task)
    group, kps, kds = S.rand_tables(ora)
    dev._tables = (kps.cuda().contiguous(), kds.cuda().contiguous(), None)      # kept alive by the env
    dev._backend.bind_actuator_rand(*dev._tables)
    for cls in S.CLASSES:
        refs = [S.rand_reference(task, cls, g) for g in range(S.RAND_GROUPS)]
        for r in refs[1:]:
            assert all(torch.equal(r.start[k], refs[0].start[k]) for k in r.start)
        hip = simulate_from(refs[0], dev)
        for g, ref in enumerate(refs):
            with S.model_gains(ref.ora, ref.gains[0], ref.gains[1]):     # (a forced re-run needs the table's gains)
                compare(ref, hip, f"{task} rand table {g}", keep=group == g)
        # not vacuous: the tables give different physics
        assert not torch.equal(refs[0].t64["dof_vel"], refs[1].t64["dof_vel"])


def test_explicit_torque_control_on_branch_states(gpu):
    """Control type "T" (ctrl != LGX_CTRL_POS_DRIVE: the torques are an input) on class A, D and G
    rows.  lgx_simulate reads caller-provided torques in that mode, as lgxo_simulate does, so the
    derived tolerance applies to 4 substeps with the torques held; and one env step against the oracle
    at the bands of test_explicit_torque_control_matches_oracle."""
    task = "go1_flat_bench"
    dev = device_env(task, S.torque_overrides)
    for cls in "ADG":
        ref = S.torque_reference(task, cls)
        ora = ref.ora
        assert ora._lgx_params.control_type == dev._lgx_params.control_type != 0
        hip = simulate_from(ref, dev)
        assert torch.equal(hip["torques"], ref.start["torques"]), "the torques are an input in this mode"
        compare(ref, hip, f"{task} ctrl=T")
        # one env step from the same start: actions that give the same torques
        S.load_start(ref)
        sync(ora, dev)
        a = ref.start["torques"] / ora.cfg.control.action_scale
        assert a.abs().max() <= ora.cfg.normalization.clip_actions
        ora.common_step_counter = dev.common_step_counter = 5
        ora.step(a.clone())
        dev.step(a.cuda())
        torch.cuda.synchronize()
        assert torch.equal(ora.torques, ref.start["torques"])
        ok, e = close(dev.torques, ora.torques, 1e-3, 1e-3)
        assert ok, f"class {cls}: torques max err {e}"
        assert (dev.torques.abs() <= dev.torque_limits + 1e-4).all()
        assert torch.equal(dev.reset_buf.cpu(), ora.reset_buf), cls
        ok, e = close(dev.dof_state, ora.dof_state, 5e-3, 2e-3)
        assert ok, f"class {cls}: dof max err {e}"
        ok, e = close(dev.obs_buf, ora.obs_buf, 5e-3, 5e-3)
        assert ok, f"class {cls}: obs max err {e}"
