"""CPU: the branch states of tests/physics_branch_states.py reach what they are built for, judged
by the float64 oracle's own decision records - so the GPU comparison on these states
(tests/test_gpu_physics_branches.py) cannot pass vacuously - and no constructed decision sits
within rounding of its threshold, where float32 could take the other branch.

Run with -s for the coverage table and the float32 oracle's errors against float64."""
import pytest
import torch

import physics_branch_states as S
from test_gpu_parity import BRANCH_MARGIN_MAX

TASKS = ["go1_flat_bench", "go1_rough", "aliengo", "a1", "cassie"]
CLAMP_MARGIN = 1e-3     # relative distance of the unclamped velocity to dof_vel_limit


def _joints(task, limited_only=True):
    return set(range(12)) - (S.FREE_JOINTS.get(task, set()) if limited_only else set())


def _first(limit, decision):
    """{joint: first substep with `decision`} of a coverage's limit set."""
    out = {}
    for j, d, s in limit:
        if d == decision:
            out[j] = min(s, out.get(j, S.NSUB))
    return out


@pytest.mark.parametrize("task", TASKS)
def test_free_joints_are_the_listed_ones(task):
    a = S.model_arrays(S.oracle_env(task))
    assert {j for j in range(12) if not a.lo[j] < a.hi[j]} == S.FREE_JOINTS.get(task, set())
    assert (a.vl > 0).all() and (a.eff > 0).all()


@pytest.mark.parametrize("task", TASKS)
def test_limit_classes_reach_every_decision_on_every_joint(task):
    want = _joints(task)
    cov = {c: S.reference(task, c).cov for c in "ABCE"}
    for d in (-1, 1):                                   # A: outside from the first substep on
        assert {j for j, s in _first(cov["A"].limit, d).items() if s == 0} == want, ("A", d)
        got = _first(cov["B"].limit, d)                 # B: inside first, outside in a later substep
        assert set(got) == want and all(s >= 1 for s in got.values()), ("B", d, got)
        assert {j for j, dd, s in cov["C"].limit if dd == d and s == 0} == want, ("C", d)
        got = _first(cov["E"].limit, d)
        assert set(got) == want and all(s >= 1 for s in got.values()), ("E", d, got)
    assert {j for j, s in _first(cov["B"].limit, 0).items() if s == 0} == want
    back = _first(cov["C"].limit, 0)                    # C: inside again before the last substep
    assert set(back) == want and all(1 <= s <= S.NSUB - 1 for s in back.values()), back
    # row by row: the decision of a B / C row changes after the first substep
    for c in "BC":
        r = S.reference(task, c)
        for e in (r.plan.joint >= 0).nonzero().flatten().tolist():
            seq = [r.decisions[(e, s, 2, int(r.plan.joint[e]))] for s in range(S.NSUB)]
            side = int(r.plan.side[e])
            assert len(seq) == S.NSUB and seq[0] == (0 if c == "B" else side) and (side if c == "B" else 0) in seq[1:], (c, e, seq)


@pytest.mark.parametrize("task", TASKS)
def test_every_joint_saturates_with_both_signs_and_runs_implicit(task):
    r = S.reference(task, "F")
    for e in (r.plan.joint >= 0).nonzero().flatten().tolist():     # each F row saturates its joint, its sign, at once
        j, s = int(r.plan.joint[e]), int(r.plan.side[e])
        assert r.decisions[(e, 0, 1, j)] == 0, e
        assert float(r.outs[0]["torques"][e, j]) == s * float(S.model_arrays(r.ora).eff[j]), (e, j)
    for what in ("+sat", "-sat"):
        assert {j for j, w in r.cov.drive if w == what} == set(range(12)), what
    assert {j for j, w in r.cov.any_drive if w == "implicit"} == set(range(12))


@pytest.mark.parametrize("task", TASKS)
def test_every_joint_is_clamped_at_both_velocity_limits(task):
    for c in "DE":
        r = S.reference(task, c)
        rows = (r.plan.joint >= 0).nonzero().flatten().tolist()
        assert len(rows) == 4 * len(_joints(task, limited_only=c == "E"))
        own = [x for x in r.cov.clamp if int(r.plan.joint[x[0]]) == x[1]]
        assert {x[0] for x in own} == set(rows), f"{c}: rows that never end a substep at the clamp"
        for e, j, s, sign in own:
            assert sign == int(r.plan.side[e])
        for sign in (-1, 1):
            assert {x[1] for x in own if x[3] == sign} == _joints(task, limited_only=c == "E"), (c, sign)
        if c == "E":     # the same rows run into the limit afterwards
            for e in rows:
                seq = [r.decisions[(e, s, 2, int(r.plan.joint[e]))] for s in range(S.NSUB)]
                assert seq[0] == 0 and int(r.plan.side[e]) in seq[1:], (e, seq)


@pytest.mark.parametrize("task", TASKS)
def test_limit_under_contact_load(task):
    """Class G: every joint with limits is past a limit in a substep in which a candidate of its own
    leg penetrates, and both sides occur; Go1's calves at their lower stop (-2.723) among them."""
    r = S.reference(task, "G")
    assert {j for j, _ in r.cov.load} == _joints(task), sorted(r.cov.load)
    assert {d for _, d in r.cov.load} == {-1, 1}
    if task.startswith("go1"):
        assert {(j, -1) for j in (2, 5, 8, 11)} <= r.cov.load
    rows = (r.plan.joint >= 0).nonzero().flatten()
    assert r.t64["contact_forces"][rows].abs().amax((1, 2)).gt(0).sum() >= len(rows) // 2


@pytest.mark.parametrize("task", TASKS)
def test_no_constructed_decision_is_within_rounding_of_its_threshold(task):
    for c in S.CLASSES:
        r = S.reference(task, c)
        near = S.near_threshold(r.plan, r.records, BRANCH_MARGIN_MAX)     # any substep, not only the placed one
        assert not near, f"class {c}: {near}"
        if c in "DE":
            a = S.model_arrays(r.ora)
            for e in (r.plan.joint >= 0).nonzero().flatten().tolist():
                j = int(r.plan.joint[e])
                for s, o in enumerate(r.outs):
                    rel = abs(abs(float(o["unclamped"][e, j])) / float(a.vl[j]) - 1.0)
                    assert rel > CLAMP_MARGIN, f"class {c} env {e} joint {j} substep {s}: unclamped velocity {rel:.2e} from the limit"


@pytest.mark.parametrize("task", TASKS)
def test_float32_oracle_is_finite_and_not_exact(task):
    """check_derived measures HIP against the float32 oracle's error: that error must exist (not the
    floor alone) and be finite on these states.  Printed, not bounded."""
    for c in S.CLASSES:
        r = S.reference(task, c)
        errs = {k: (r.o32[k].double() - r.t64[k]).abs().max().item() for k in r.t64}
        cov = r.cov
        print(f"{task:15s} {c}: rows {int((r.plan.joint >= 0).sum()):2d}  limit -1/0/+1 "
              f"{sum(1 for x in cov.limit if x[1] < 0)}/{sum(1 for x in cov.limit if x[1] == 0)}/{sum(1 for x in cov.limit if x[1] > 0)}"
              f"  drive impl/+sat/-sat {'/'.join(str(sum(1 for x in cov.drive if x[1] == w)) for w in ('implicit', '+sat', '-sat'))}"
              f"  clamped {len(cov.clamp):3d}  load {len(cov.load):2d}  f32 err "
              + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in r.o32.items():
            assert torch.isfinite(v).all(), (c, k)
        for k in ("root_pose", "root_vel", "dof_pos", "dof_vel", "torques"):
            assert errs[k] > 0, (c, k)
        if c == "G":
            assert errs["contact_forces"] > 0


def test_per_leg_limits_variant_differs_by_leg_and_is_covered():
    """The variant with limits that differ from leg to leg (a stride error in the limit lookup is
    invisible on robots whose legs share their limits): all 12 (lower, upper) pairs distinct by leg,
    and the limit classes reach every decision on every joint away from the thresholds."""
    task = "go1_flat_bench"
    a = S.model_arrays(S.oracle_env(task, key=task + S.LEGS))
    base = S.model_arrays(S.oracle_env(task))
    leg = torch.arange(12) // 3
    assert torch.allclose(a.lo, base.lo + 0.04 * leg) and torch.allclose(a.hi, base.hi - 0.03 * leg)
    for k in range(3):
        assert len({float(x) for x in a.lo[k::3]}) == 4 and len({float(x) for x in a.hi[k::3]}) == 4
    for c in "ABCEG":
        r = S.legs_reference(task, c)
        assert not S.near_threshold(r.plan, r.records, BRANCH_MARGIN_MAX), c
        if c != "G":
            for d in (-1, 1):
                assert {j for j, dd, _ in r.cov.limit if dd == d} == set(range(12)), (c, d)
    assert {j for j, _ in S.legs_reference(task, "G").cov.load} == set(range(12))
