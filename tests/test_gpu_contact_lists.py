"""The physics kernel's contact lists (lgx_physics_kernel<PP>: every lane visits only the
penetrating ones of its own candidate slots, from a mask built once per substep) on states with
many contacts per leg and per lane.

The states are built on the CPU with the oracle alone (seeded, fixed below): bases in the air,
standing, lowered onto the ground, rolled onto a side, upside down, legs folded under, so that
legs carry 0, 1, PP, PP + 1 and >= 2 PP + 1 penetrating candidates.  The counts come from the
float64 oracle's decision records (kind 3: candidate in contact) and are asserted before any
comparison, so the tests cannot pass vacuously.  Tolerances: check_derived of test_gpu_parity
(the HIP error against the float64 truth within a multiple of the float32 oracle's)."""
import pytest
import torch

from oracle_backend import make_env
from test_gpu_parity import PHYS_QTY, STATE, check_derived, float64_truth, randomize_state, sync

pytestmark = pytest.mark.gpu

PP = 4          # the product's lane split (lgx_physics_pp)
NSUB = 4
SEED = 20
N = 64
_CACHE = {}


def contact_states(env, seed=SEED):
    """Seeded start states, by env index mod 8: 0 in the air, 1 standing, 2 base lowered onto the
    ground, 3 / 6 rolled onto a side (6 with the legs folded), 4 legs folded under the base,
    5 upside down, 7 dropped at a random attitude.
    The folded pose [0, 1.3, -2.55] +- 0.1 passes Go1's calf stop (-2.723) only where the noise
    carries it there: a few calves of the mod-4 rows (asserted in `reference`, so the claim is not
    implicit), none of the rolled mod-6 rows.  These states aim at the contact lists; a joint past a
    limit on every joint while its leg is loaded is class G of tests/physics_branch_states.py."""
    n = env.num_envs
    gen = torch.Generator().manual_seed(seed)
    randomize_state(env, gen, standing=False)
    r = lambda *s: torch.rand(*s, generator=gen)
    kind = torch.arange(n) % 8
    rs = env.root_states
    height = torch.tensor([1.0, 0.315, 0.10, 0.08, 0.06, 0.055, 0.07, 0.0])[kind] + 0.01 * (r(n) - 0.5)
    roll = torch.tensor([0.0, 0.0, 0.0, 1.5708, 0.0, 3.1416, -1.5708, 0.0])[kind] + 0.2 * (r(n) - 0.5)
    pitch = 0.2 * (r(n) - 0.5)
    yaw = 6.28 * r(n)
    cr, sr, cp, sp, cy, sy = [f(a / 2) for a in (roll, pitch, yaw) for f in (torch.cos, torch.sin)]
    quat = torch.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                        cr * cp * cy + sr * sp * sy], 1)
    fixed = kind != 7
    rs[fixed, 2] = env.env_origins[fixed, 2] + height[fixed]
    rs[fixed, 3:7] = quat[fixed]
    rs[fixed, 7:13] = (r(n, 6)[fixed] - 0.5) * 0.4
    folded = torch.tensor([0.0, 1.3, -2.55]).repeat(4)
    pose = env.default_dof_pos.expand(n, 12).clone()
    pose[(kind == 4) | (kind == 6)] = folded
    env.dof_pos[fixed] = pose[fixed] + (r(n, 12)[fixed] - 0.5) * 0.2
    env.dof_vel[fixed] = (r(n, 12)[fixed] - 0.5) * 1.0
    env.target_poses[:] = torch.clip(env.dof_pos + (r(n, 12) - 0.5) * 0.3, env.dof_pos_limits[:, 0],
                                     env.dof_pos_limits[:, 1])


def point_legs(env):
    """Leg lane of every contact candidate as the kernel deals them (lgx_sim_create: leg points to
    their leg, base points round-robin)."""
    m = env._backend.m
    legs, rr = [], 0
    for i in range(m.num_points):
        d = m.point_dyn[i]
        if d == 0:
            legs.append(rr & 3)
            rr += 1
        else:
            legs.append((d - 1) // 3)
    return legs


def leg_counts(env, records, n=N, nsub=NSUB):
    """[env, leg, substep] number of penetrating candidates in the float64 run."""
    return lane_counts(env, records, 1, n, nsub)[:, :, 0]


def lane_counts(env, records, pp=PP, n=N, nsub=NSUB):
    """[env, leg, lane, substep] number of penetrating candidates on each of the leg's `pp` lanes
    (the leg's c-th candidate sits on lane c mod pp): the trips of that lane's contact loops."""
    legs = point_legs(env)
    seen, lane = [0, 0, 0, 0], []
    for leg in legs:
        lane.append(seen[leg] % pp)
        seen[leg] += 1
    cnt = torch.zeros(n, 4, pp, nsub, dtype=torch.long)
    for e, s, kind, index, decision, _ in records:
        if kind == 3 and decision:
            cnt[e, legs[index], lane[index], s] += 1
    return cnt


def assert_not_vacuous(cnt):
    flat = cnt.reshape(-1)
    assert (flat > PP).sum() >= 8, f"legs above PP contacts: {(flat > PP).sum()}"
    assert (flat >= 2 * PP + 1).sum() >= 1, "no leg with at least 2 PP + 1 contacts"
    assert (flat == 0).sum() >= 8, "fewer than 8 legs without contact"
    for k in (1, PP, PP + 1):
        assert (flat == k).any(), f"no leg with {k} contacts"


def reference(task):
    """(oracle env in the start state, float64 truth, float32 oracle results, counts), computed once."""
    if task not in _CACHE:
        ora = make_env(task, num_envs=N, device="cpu", backend="oracle")
        contact_states(ora)
        t64 = float64_truth(ora, NSUB)
        cnt = leg_counts(ora, t64.records)
        assert_not_vacuous(cnt)
        own = lane_counts(ora, t64.records)   # what sets the trip count: contacts of one lane at PP = 4
        assert (own == 1).any() and (own == 2).sum() >= 8 and (own >= 3).sum() >= 8, "no lane with 1, 2 and >= 3 contacts"
        # limit decisions (kind 2) of these states: calves of the folded rows below their lower stop, nothing above one
        past = {(e, j) for e, _, kind, j, decision, _ in t64.records if kind == 2 and decision < 0}
        assert len(past) >= 3 and all(e % 8 == 4 and j % 3 == 2 for e, j in past), sorted(past)
        assert not any(kind == 2 and decision > 0 for _, _, kind, _, decision, _ in t64.records)
        start = {k: getattr(ora, k).clone() for k in STATE}
        ora.simulate(NSUB)
        o32 = {k: f(ora).clone() for k, f in PHYS_QTY.items()}
        for k, v in start.items():
            getattr(ora, k).copy_(v)
        _CACHE[task] = (ora, t64, o32, cnt)
    return _CACHE[task]


def run_gpu(task, ora):
    dev = make_env(task, num_envs=N, device="cuda:0", backend="lgx")
    sync(ora, dev)
    if hasattr(ora, "terrain_types"):
        dev.terrain_types.copy_(ora.terrain_types)
    dev.simulate(NSUB)
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize("task", ["go1_rough", "go1_flat_bench"])
def test_many_contacts_per_leg_match_float64(gpu, task):
    """Legs with 0 .. >= 2 PP + 1 penetrating candidates: every physics quantity (contact forces
    included) within the derived tolerance of the float64 truth."""
    ora, t64, o32, _ = reference(task)
    dev = run_gpu(task, ora)
    check_derived(t64, o32, {k: f(dev) for k, f in PHYS_QTY.items()})


@pytest.mark.parametrize("pp", ["1", "2", "4", "8"])
@pytest.mark.parametrize("task", ["go1_rough", "go1_flat_bench"])
def test_every_lane_split(gpu, monkeypatch, task, pp):
    """The same states under every LGX_PHYS_PP (1: the whole leg on one lane; 8: two DPP rows per env)."""
    monkeypatch.setenv("LGX_PHYS_PP", pp)
    ora, t64, o32, _ = reference(task)
    dev = run_gpu(task, ora)
    check_derived(t64, o32, {k: f(dev) for k, f in PHYS_QTY.items()})


def _outputs(dev):
    out = {"root_states": dev.root_states, "dof_state": dev.dof_state.reshape(-1, 24), "torques": dev.torques,
           "contact_forces": dev._contact_forces_full}
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _layout(dev, ora, rows):
    """Env i of `dev` takes the state of env rows[i] of `ora`."""
    idx = torch.as_tensor(rows)
    for name in STATE:
        s, d = getattr(ora, name), getattr(dev, name)
        if name == "_episode_sums_buf":      # [terms, envs]
            d.copy_(s[:, idx].to(d.device))
        elif name == "dof_state":            # [envs * 12, 2]
            d.copy_(s.reshape(N, 12, 2)[idx].reshape(-1, 2).to(d.device))
        else:
            d.copy_(s[idx].to(d.device))
    if hasattr(ora, "actuator_history"):
        dev.actuator_history.copy_(ora.actuator_history[idx].to(dev.actuator_history.device))


def test_leg_result_does_not_depend_on_neighbours(gpu):
    """50 envs on the plane (task go1: the plane with the actuator net, so a full step writes
    model_ins; a ragged last workgroup; 4 envs per wave) that are copies of 5 states with 0 .. many
    contacts per leg, in three layouts: every output row is bitwise the row of the same state in the
    other layout, and a layout repeated is bitwise itself."""
    ora, _, _, cnt = reference("go1")
    per_env = cnt.amax((1, 2))
    picks = [int(torch.nonzero(c)[0]) for c in (per_env == 0, per_env == 1, (per_env > 1) & (per_env <= PP),
                                                 (per_env > PP) & (per_env < 2 * PP + 1), per_env >= 2 * PP + 1)]
    n = 50
    gen = torch.Generator().manual_seed(3)
    lay_a = [picks[i % 5] for i in range(n)]                       # a b c d e a b c d e ...
    lay_b = [picks[(i // 4 + (i % 4 == 3)) % 5] for i in range(n)]  # three envs of a wave alike, the fourth not
    lay_c = [picks[i] for i in torch.randint(0, 5, (n,), generator=gen).tolist()]
    dev = make_env("go1", num_envs=n, device="cuda:0", backend="lgx")
    a_act = (torch.rand(N, 12, generator=gen) - 0.5) * 2

    def run(rows):
        _layout(dev, ora, rows)
        dev.simulate(NSUB)
        torch.cuda.synchronize()
        out = _outputs(dev)
        _layout(dev, ora, rows)   # model_ins: the actuator-net rows the physics launch of a full step writes
        dev.step(a_act[torch.as_tensor(rows)].cuda())
        torch.cuda.synchronize()
        out["model_ins"] = dev._model_ins_all.detach().cpu().clone().transpose(0, 1)
        return out

    res = {name: run(rows) for name, rows in (("a", lay_a), ("b", lay_b), ("c", lay_c), ("a2", lay_a))}
    for k in res["a"]:
        assert torch.equal(res["a"][k], res["a2"][k]), f"{k}: two runs of one layout differ"
    first = {s: lay_a.index(s) for s in picks}
    for name, rows in (("b", lay_b), ("c", lay_c)):
        for k, v in res[name].items():
            want = res["a"][k][torch.as_tensor([first[s] for s in rows])]
            bad = [i for i in range(n) if not torch.equal(v[i], want[i])]
            assert not bad, f"{k}: layout {name} rows {bad} differ from the same state's row in layout a"
    assert res["a"]["contact_forces"].abs().sum() > 0 and res["a"]["model_ins"].abs().sum() > 0


def test_report_routing(gpu):
    """Envs where a leg's foot and calf both penetrate and the base touches: every body the float64
    truth reports a force for is non-zero on the GPU (and within the derived bound, test 1), every
    other body exactly zero."""
    ora, t64, o32, _ = reference("go1_flat_bench")
    m = ora._backend.m
    hit = torch.zeros(N, NSUB, len(PHYS_QTY["contact_forces"](ora)[0]), dtype=torch.bool)
    for e, s, kind, index, decision, _ in t64.records:
        if kind == 3 and decision:
            hit[e, s, m.point_report[index]] = True
    last = hit[:, NSUB - 1]
    feet = [4 + 4 * leg for leg in range(4)]
    both = torch.stack([last[:, f] & last[:, f - 1] for f in feet], 1).any(1) & last[:, 0]
    assert both.sum() >= 1, "no env with foot + calf of one leg and the base in contact"
    dev = run_gpu("go1_flat_bench", ora)
    f64 = t64["contact_forces"]
    gpu_f = PHYS_QTY["contact_forces"](dev).detach().cpu().double()
    nz64, nzg = f64.abs().amax(2) > 0, gpu_f.abs().amax(2) > 0
    rows = torch.nonzero(both).reshape(-1)
    assert (nz64[rows].sum(1) >= 3).all()
    assert torch.equal(nz64[rows], nzg[rows]), "bodies with a reported force differ from the float64 truth"
    check_derived(t64, o32, {k: f(dev) for k, f in PHYS_QTY.items()}, keep=both, qty=["contact_forces"])


def test_anymal_lowered_bases(gpu):
    """ANYmal C on rough terrain (every candidate a sphere: the corrected-trimesh queue feeds the
    lists), one seed of test_physics_rough_terrain_derived_tolerance's recipe with the bases lowered."""
    ora = make_env("anymal_c_rough", num_envs=N, device="cpu", backend="oracle")
    dev = make_env("anymal_c_rough", num_envs=N, device="cuda:0", backend="lgx")
    gen = torch.Generator().manual_seed(100)
    randomize_state(ora, gen, standing=True)
    ora.root_states[:, 2] -= 0.25 * torch.rand(N, generator=gen) + 0.05
    sync(ora, dev)
    dev.terrain_types.copy_(ora.terrain_types)
    t64 = float64_truth(ora, NSUB)
    cnt = leg_counts(ora, t64.records)
    assert (cnt > PP).sum() >= 8 and (cnt > 0).sum() >= 64, "too few contacts to exercise the lists"
    ora.simulate(NSUB)
    dev.simulate(NSUB)
    torch.cuda.synchronize()
    check_derived(t64, {k: f(ora) for k, f in PHYS_QTY.items()}, {k: f(dev) for k, f in PHYS_QTY.items()})
