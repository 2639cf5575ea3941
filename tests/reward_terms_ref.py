"""A float64 reference of one `post_physics_step`'s termination, reward terms, episode sums and
extras, the deterministic state it is checked on, and the test body the CPU (oracle) and GPU (HIP
kernel) tests share.

The reference restates the semantics of the reference project's LeggedRobot (post_physics_step,
_post_physics_step_callback's heading command, check_termination, compute_reward, every _reward_*,
the episode means of reset_idx; Cassie's _reward_no_fly) in plain numpy float64.  It is written from
those semantics, not from lgx_envlogic.hip or lgx_oracle.c, and reads nothing of the package but the
names of the terms.  The env hands over index lists, limits, scales and dt (params_from_env).

Inputs: the state as the kernel reads it, captured before the step, and three sets of device
outputs published by the step: measured_heights (the height scan is not restated here), and
base_lin_vel / base_ang_vel / projected_gravity.  The rotated vectors are first checked on their
own against a float64 quat_rotate_inverse (ROT_ULPS float32 ulps of the input vector's norm) and
then enter the terms as the float32 values they are, so no per-term bound carries the rotation.

Thresholds the reference project writes as Python floats are compared by torch in the tensor's
float32: 0.1 is float32(0.1) here (collision, no_fly, the command norm), the others are exact.

Error bounds (u = 2**-24, the float32 unit roundoff).  A term that is a float32 sum of n addends,
each made with k rounding errors (counted with their amplification: a square doubles what its
operand carries), times the scale, is within

    C(n, k) * u * sum_i |m_i| * |scale|,   C(n, k) = 2 * (n - 1 + k + 1),

of the float64 value: n - 1 for the sequential sum, 1 for the product with the scale, the factor 2
for fma contraction and second-order terms.  m_i is the addend, or where the addend is a
difference of a computed operand, the magnitude of the operands before they cancel.  No C may
exceed C_CAP = 64.  (n, k) per term:

    lin_vel_z            1, 1    square
    ang_vel_xy           2, 1
    orientation          2, 1
    torques             12, 1
    dof_vel             12, 1
    energy              12, 3    product (1), squared (2 + 1)
    dof_acc             12, 5    difference, quotient by dt (2), squared (4 + 1)
    action_rate         12, 3    difference (1), squared (2 + 1)
    dof_pos_limits      12, 2    difference to a limit, sum of the two clipped parts
    dof_vel_limits      12, 2    limit * soft factor, difference; m = |v| + limit * soft
    torque_limits       12, 2    the same with torques
    feet_air_time       nf, 2    t + dt, minus 0.5; m = t + dt + 0.5
    stand_still         12, 1    |q - default| (the 0 / 1 factor is exact)
    hip_motion           4, 1
    feet_contact_forces nf, 4    3-vector norm (the sum of squares carries 3, the root halves it
                                 and adds 1: <= 3), difference (1); m = |F| + max_contact_force
    base_height          P, 1    mean over P scan points of (z - h_i): the sum, then one quotient;
                                 d = mean - target carries dm = C * u * mean|z - h_i| + u |d|, the
                                 square 2 |d| dm + u d**2 - relative to the addends, not to the
                                 tiny result.  Without a height scan the mean is root z itself.
                                 P = 187 would give C = 378: the sequential float32 sum's worst case.
                                 It is held to C_CAP instead, which rounding errors that do not all
                                 point the same way keep with a wide margin (their sum grows with
                                 sqrt(P): 4 * sqrt(186) = 55); the measured ratio is in DESIGN.md.
    tracking_lin_vel     argument (ex**2 + ey**2) / sigma: 2 addends of k = 3, one quotient:
                         da = 2 * (1 + 3 + 1) * u * a; value e**-a: da * value + 2 ulp (expf)
    tracking_ang_vel     ez = cmd_yaw - w_z with cmd_yaw from the heading: the forward vector
                         (quat_apply, K_QUAT = 32 roundings of operands <= 2 per component), atan2f
                         (2 ulp), the difference to the heading command, the wrap (one rounding of a
                         value <= 2 pi, twice, and float32(2 pi) against 2 pi), halved and clipped;
                         da = (2 |ez| dez + 2 * 2 u ez**2) / sigma; value as above
    collision, stumble, no_fly, termination    counts and booleans: exact

What is compared is float32(start + float32(term * scale)) per episode-sum row, bound: the above
plus one rounding u * |row|; with a zero start the exact terms' rows must equal float32(count *
scale) bit for bit.  rew_buf: the terms' bounds plus the float32 sum of the T products in
reward_names order, C(T, 0) - 2 (no scale product), the clip (1-Lipschitz), one rounding for the
termination addend.  Extras: the reset envs' bounds summed plus the float32 sum over the R reset
envs in whatever order (block partials, a butterfly), the quotients by R and max_episode_length_s:
C(R, 1).
"""
import numpy as np

from legged_gym_amd.sim.abi import MAX_TERMS, REWARD_IDS

U = 2.0 ** -24
C_CAP = 64
ROT_ULPS = 64          # tests/test_gpu_parity.py PHYS_ULPS
K_QUAT = 32
MARGIN_MIN = 1e-4      # a condition on the random rows, not a tolerance
N_ENVS = 77            # four full 16-env post-physics workgroups and a 13-env tail
THR01 = float(np.float32(0.1))
TWO_PI_ERR = abs(float(np.float32(2 * np.pi)) - 2 * np.pi)
ALL_TERMS = [n for n in REWARD_IDS if n != "termination"]
EXACT_TERMS = ("collision", "stumble", "no_fly", "termination")
# every term's per-step product (term * scale * dt, dt = 0.02) comes to 1e-2 .. 1e2 on the builder's rows
ALL_SCALES = {
    "lin_vel_z": -100., "ang_vel_xy": -100., "orientation": -100., "base_height": -2000., "torques": -0.05,
    "energy": -0.00125, "dof_vel": -0.15, "dof_acc": -5e-5, "action_rate": -5., "collision": -20.,
    "termination": -100., "dof_pos_limits": -500., "dof_vel_limits": -50., "torque_limits": -20.,
    "tracking_lin_vel": 2000., "tracking_ang_vel": 2000., "feet_air_time": 100., "stumble": -50.,
    "stand_still": -25., "feet_contact_forces": -2., "hip_motion": -50., "no_fly": 50.,
}
assert set(ALL_SCALES) == set(REWARD_IDS)


def C_nk(n, k):
    c = 2 * (n - 1 + k + 1)
    assert c <= C_CAP, (n, k)
    return c


def _f(a):
    return np.asarray(a, dtype=np.float64)


def quat_rotate_inverse(q, v):
    qw, qv = q[:, 3:4], q[:, :3]
    return v * (2.0 * qw ** 2 - 1.0) - np.cross(qv, v) * qw * 2.0 + qv * np.sum(qv * v, axis=1, keepdims=True) * 2.0


def quat_apply(q, v):
    t = np.cross(q[:, :3], v) * 2.0
    return v + q[:, 3:4] * t + np.cross(q[:, :3], t)


def decide(lhs, thr):
    """(relative distance of lhs to thr, both sides exactly float32 values)."""
    lhs, thr = np.broadcast_arrays(_f(lhs), _f(thr))
    den = np.maximum(np.abs(lhs), np.abs(thr))
    margin = np.where(den > 0, np.abs(lhs - thr) / np.where(den > 0, den, 1.0), 0.0)
    exact = (lhs.astype(np.float32).astype(np.float64) == lhs) & (thr.astype(np.float32).astype(np.float64) == thr)
    return margin, exact


# ---------------------------------------------------------------------------------- parameters
def params_from_env(env):
    """What the env hands over: index lists, limits, scales (as the float32 the kernels read) and dt."""
    cfg, f32 = env.cfg, lambda x: float(np.float32(x))
    t = lambda x: x.detach().cpu().numpy()
    rows = env.reward_names + (["termination"] if "termination" in env.reward_scales else [])
    return dict(
        dt=f32(env.dt), names=list(env.reward_names), rows=rows,
        scales={k: f32(v) for k, v in env.reward_scales.items()},
        only_positive=bool(cfg.rewards.only_positive_rewards), sigma=f32(cfg.rewards.tracking_sigma),
        base_height_target=f32(cfg.rewards.base_height_target), max_contact_force=f32(cfg.rewards.max_contact_force),
        soft_lower=_f(t(env.dof_pos_limits[:, 0])), soft_upper=_f(t(env.dof_pos_limits[:, 1])),
        dof_vel_limits=_f(t(env.dof_vel_limits)), soft_dof_vel_limit=f32(cfg.rewards.soft_dof_vel_limit),
        torque_limits=_f(t(env.torque_limits)), soft_torque_limit=f32(cfg.rewards.soft_torque_limit),
        default_dof_pos=_f(t(env.default_dof_pos[0])), feet=t(env.feet_indices).tolist(),
        penalised=t(env.penalised_contact_indices).tolist(), termination=t(env.termination_contact_indices).tolist(),
        max_episode_length=float(env.max_episode_length), max_episode_length_s=f32(env.max_episode_length_s),
        measure_heights=bool(cfg.terrain.measure_heights), heading_command=bool(cfg.commands.heading_command),
        resample_interval=int(cfg.commands.resampling_time / env.dt), num_bodies=int(env.num_bodies),
        env_origins=t(env.env_origins).copy())


# ---------------------------------------------------------------------------------- the reference
def rotation_check(s, par):
    """{name: (float64 value, bound)} of base_lin_vel, base_ang_vel, projected_gravity."""
    rs = _f(s["root_states"])
    q = rs[:, 3:7]
    out = {}
    for name, v in (("base_lin_vel", rs[:, 7:10]), ("base_ang_vel", rs[:, 10:13]),
                    ("projected_gravity", np.tile([0.0, 0.0, -1.0], (rs.shape[0], 1)))):
        out[name] = (quat_rotate_inverse(q, v), ROT_ULPS * 2.0 ** -23 * np.linalg.norm(v, axis=1, keepdims=True))
    return out


def reference(s, dev, par):
    """s: the state before the step; dev: measured_heights, base_lin_vel, base_ang_vel,
    projected_gravity as the step published them (float32).  Returns a dict: terms {name: (value,
    bound)} before the scale, prod / prod_bound {row name: ...} after it, rew / rew_bound / pre_clip,
    reset / time_out, feet_air_time, branches {decision: (branch, margin, exact)}."""
    rs, cf = _f(s["root_states"]), _f(s["contact_forces"])
    q, dq, tq = _f(s["dof_pos"]), _f(s["dof_vel"]), _f(s["torques"])
    cmd = _f(s["commands"])
    blv, bav, pg = _f(dev["base_lin_vel"]), _f(dev["base_ang_vel"]), _f(dev["projected_gravity"])
    N, dt = rs.shape[0], par["dt"]
    feet, nf = par["feet"], len(par["feet"])
    fat = _f(s["feet_air_time"])[:, :nf]
    br, terms = {}, {}

    def sum_term(name, addends, k, mags=None):
        addends = _f(addends)
        mags = np.abs(addends) if mags is None else _f(mags)
        terms[name] = (addends.sum(axis=1), C_nk(addends.shape[1], k) * U * mags.sum(axis=1))

    # _post_physics_step_callback: the yaw command from the heading error
    if par["heading_command"]:
        fwd = quat_apply(rs[:, 3:7], np.tile([1.0, 0.0, 0.0], (N, 1)))
        heading = np.arctan2(fwd[:, 1], fwd[:, 0])
        diff = cmd[:, 3] - heading
        wraps = np.round(diff / (2 * np.pi))
        wrapped = diff - 2 * np.pi * wraps
        m, _ = decide(np.abs(diff), np.pi)
        br["heading_wrap"] = (wraps.astype(int), m, np.zeros(N, bool))
        cmd2 = np.clip(0.5 * wrapped, -1.0, 1.0)
        br["yaw_command_clip"] = ((np.abs(0.5 * wrapped) > 1.0).astype(int), None, None)
        d_heading = K_QUAT * np.sqrt(2.0) * U / np.hypot(fwd[:, 0], fwd[:, 1]) + 4 * U * np.abs(heading)
        d_cmd2 = 0.5 * (d_heading + U * np.abs(diff) + 2 * U * 2 * np.pi + TWO_PI_ERR)
    else:
        cmd2, d_cmd2 = cmd[:, 2], np.zeros(N)
    cmd_norm = np.hypot(cmd[:, 0], cmd[:, 1])
    m, ex = decide(cmd_norm, THR01)
    br["command_norm"] = (np.where(cmd_norm > THR01, 1, np.where(cmd_norm < THR01, -1, 0)), m, ex)

    # check_termination
    Ft = np.linalg.norm(cf[:, par["termination"], :], axis=-1)
    m, ex = decide(Ft, 1.0)
    br["termination_contact"] = ((Ft > 1.0).astype(int), m, ex)
    ep = np.asarray(s["episode_length"], np.int64) + 1
    time_out = ep > par["max_episode_length"]
    m, ex = decide(ep, par["max_episode_length"])
    br["time_out"] = (time_out.astype(int), m, ex)
    reset = (Ft > 1.0).any(axis=1) | time_out
    br["reset_kind"] = ((Ft > 1.0).any(axis=1) * 1 + time_out * 2, None, None)

    # the terms
    sum_term("lin_vel_z", blv[:, 2:3] ** 2, 1)
    sum_term("ang_vel_xy", bav[:, :2] ** 2, 1)
    sum_term("orientation", pg[:, :2] ** 2, 1)
    z = rs[:, 2]
    if par["measure_heights"]:
        a = z[:, None] - _f(dev["measured_heights"])
        P = a.shape[1]
        mean = a.mean(axis=1)
        d_mean = min(2 * (P - 1 + 1 + 1), C_CAP) * U * np.abs(a).mean(axis=1)
    else:
        mean, d_mean = z, np.zeros(N)
    d = mean - par["base_height_target"]
    dd = d_mean + U * np.abs(d)
    terms["base_height"] = (d ** 2, 2 * (2 * np.abs(d) * dd + U * d ** 2))
    sum_term("torques", tq ** 2, 1)
    sum_term("energy", (tq * dq) ** 2, 3)
    sum_term("dof_vel", dq ** 2, 1)
    sum_term("dof_acc", ((_f(s["last_dof_vel"]) - dq) / dt) ** 2, 5)
    sum_term("action_rate", (_f(s["last_actions"]) - _f(s["actions"])) ** 2, 3)
    Fp = np.linalg.norm(cf[:, par["penalised"], :], axis=-1)
    m, ex = decide(Fp, THR01)
    br["collision"] = ((Fp > THR01).astype(int), m, ex)
    terms["collision"] = ((Fp > THR01).sum(axis=1).astype(np.float64), np.zeros(N))
    terms["termination"] = ((reset & ~time_out).astype(np.float64), np.zeros(N))
    lo, hi = q - par["soft_lower"], q - par["soft_upper"]
    sum_term("dof_pos_limits", -np.minimum(lo, 0.0) + np.maximum(hi, 0.0), 2)
    br["dof_pos_limit"] = (np.where(lo < 0, -1, np.where(hi > 0, 1, 0)), None, None)
    br["dof_pos_on_limit"] = (np.where(lo == 0, -1, np.where(hi == 0, 1, 0)), None, None)
    Lv = par["dof_vel_limits"] * par["soft_dof_vel_limit"]
    xv = np.abs(dq) - Lv
    sum_term("dof_vel_limits", np.clip(xv, 0.0, 1.0), 2, np.abs(dq) + Lv)
    knee = np.abs(xv - 1.0) <= 2.0 ** -19    # limit * soft + 1 need not be a float32 number: the nearest one counts
    br["dof_vel_limit"] = (np.where(xv < 0, -1, np.where(xv == 0, 0, np.where(knee, 2, np.where(xv < 1, 1, 3)))),
                           None, None)
    Lt = par["torque_limits"] * par["soft_torque_limit"]
    xt = np.abs(tq) - Lt
    sum_term("torque_limits", np.maximum(xt, 0.0), 2, np.abs(tq) + Lt)
    on = np.abs(tq).astype(np.float32) == Lt.astype(np.float32)   # "at" the limit as float32 rounds the product
    br["torque_limit"] = (np.where(on, 0, np.where(xt > 0, 1, -1)), None, None)

    def tracking(arg, d_arg):
        val = np.exp(-arg)
        return val, d_arg * val + 4 * U * val
    ex_, ey_ = cmd[:, 0] - blv[:, 0], cmd[:, 1] - blv[:, 1]
    a = (ex_ ** 2 + ey_ ** 2) / par["sigma"]
    terms["tracking_lin_vel"] = tracking(a, 2 * (1 + 3 + 1) * U * a)
    ez = cmd2 - bav[:, 2]
    dez = d_cmd2 + U * np.abs(ez)
    terms["tracking_ang_vel"] = tracking(ez ** 2 / par["sigma"], (2 * np.abs(ez) * dez + 4 * U * ez ** 2) / par["sigma"])

    Fz = cf[:, feet, 2]
    contact = Fz > 1.0
    m, ex = decide(Fz, 1.0)
    br["contact"] = (contact.astype(int), m, ex)
    m, ex = decide(fat, 0.0)
    br["air_time_positive"] = ((fat > 0).astype(int), m, ex)
    first = (fat > 0) & contact
    br["first_contact"] = (first.astype(int), None, None)
    fat1 = fat + dt
    moving = (cmd_norm > THR01)[:, None]
    sum_term("feet_air_time", (fat1 - 0.5) * first * moving, 2, (fat1 + 0.5) * first * moving)
    fat_after = fat1 * ~contact if "feet_air_time" in par["names"] else fat.copy()   # the term itself keeps the clock
    fat_after[reset] = 0.0
    Fxy = np.hypot(cf[:, feet, 0], cf[:, feet, 1])
    m, ex = decide(Fxy, 5 * np.abs(Fz))
    br["stumble"] = ((Fxy > 5 * np.abs(Fz)).astype(int), m, ex)
    terms["stumble"] = ((Fxy > 5 * np.abs(Fz)).any(axis=1).astype(np.float64), np.zeros(N))
    sum_term("stand_still", np.abs(q - par["default_dof_pos"]) * (cmd_norm < THR01)[:, None], 1)
    Ff = np.linalg.norm(cf[:, feet, :], axis=-1)
    xf = Ff - par["max_contact_force"]
    sum_term("feet_contact_forces", np.maximum(xf, 0.0), 4, Ff + par["max_contact_force"])
    br["contact_force_limit"] = (np.sign(xf).astype(int), None, None)
    hips = [0, 3, 6, 9]
    sum_term("hip_motion", np.abs(q[:, hips] - par["default_dof_pos"][hips]), 1)
    m, ex = decide(Fz, THR01)
    br["no_fly_contact"] = ((Fz > THR01).astype(int), m, ex)
    terms["no_fly"] = (((Fz > THR01).sum(axis=1) == 1).astype(np.float64), np.zeros(N))

    # compute_reward
    prod, prod_bound = {}, {}
    for name in par["rows"]:
        v, b = terms[name]
        sc = par["scales"][name]
        prod[name] = v * sc
        prod_bound[name] = (b * abs(sc) if name not in EXACT_TERMS else U * np.abs(v * sc))
    T = len(par["names"])
    pre = sum((prod[n] for n in par["names"]), np.zeros(N))
    rew_bound = sum((prod_bound[n] for n in par["names"]), np.zeros(N))
    if T > 1:
        rew_bound = rew_bound + 2 * (T - 1) * U * sum(np.abs(prod[n]) for n in par["names"])
    rew = np.maximum(pre, 0.0) if par["only_positive"] else pre.copy()
    br["positive_clip"] = ((pre < 0).astype(int), None, None)
    if "termination" in par["scales"]:
        rew = rew + prod["termination"]
        rew_bound = rew_bound + prod_bound["termination"] + U * np.abs(rew)
    return dict(terms=terms, prod=prod, prod_bound=prod_bound, rew=rew, rew_bound=rew_bound, pre_clip=pre,
                reset=reset, time_out=time_out, episode_length=np.where(reset, 0, ep), feet_air_time=fat_after,
                branches=br, cmd2=cmd2)


# decisions whose two sides give different values (a margin is needed), and the terms that read them
DISCONTINUOUS = {"heading_wrap": ("tracking_ang_vel",), "command_norm": ("feet_air_time", "stand_still"),
                 "termination_contact": (), "time_out": (), "collision": ("collision",),
                 "contact": ("feet_air_time",), "air_time_positive": ("feet_air_time",), "stumble": ("stumble",),
                 "no_fly_contact": ("no_fly",)}
# every branch a case must take in >= 2 envs, by the terms that make it matter (() = always)
BRANCHES = {"heading_wrap": ((-1, 0, 1), ("tracking_ang_vel",)), "command_norm": ((-1, 0, 1), ("feet_air_time", "stand_still")),
            "termination_contact": ((0, 1), ()), "time_out": ((0, 1), ()), "reset_kind": ((0, 1, 2, 3), ()),
            "collision": ((0, 1), ("collision",)), "contact": ((0, 1), ("feet_air_time",)),
            "air_time_positive": ((0, 1), ("feet_air_time",)), "first_contact": ((0, 1), ("feet_air_time",)),
            "stumble": ((0, 1), ("stumble",)), "no_fly_contact": ((0, 1), ("no_fly",)),
            "dof_pos_limit": ((-1, 0, 1), ("dof_pos_limits",)), "dof_pos_on_limit": ((-1, 1), ("dof_pos_limits",)),
            "dof_vel_limit": ((-1, 0, 1, 2, 3), ("dof_vel_limits",)), "torque_limit": ((-1, 0, 1), ("torque_limits",)),
            "contact_force_limit": ((-1, 0, 1), ("feet_contact_forces",)), "positive_clip": ((0, 1), ())}
# decisions a hand-placed row puts exactly on the threshold (margin 0, both sides float32 values)
ON_THRESHOLD = ("command_norm", "contact", "no_fly_contact", "air_time_positive", "time_out", "termination_contact", "stumble")


def min_margin(ref, rows, names):
    """The smallest relative margin over the discontinuous decisions the active terms read, on
    `rows`; a decision whose two sides are exactly float32 values (a single component, an
    axis-aligned power-of-two vector: every float32 evaluation gives them exactly) has no
    rounding to cross and counts as safe."""
    worst = (np.inf, None)
    for dec, m in env_margins(ref, names).items():
        if m[rows].size and m[rows].min() < worst[0]:
            worst = (float(m[rows].min()), dec)
    return worst


def env_margins(ref, names):
    """{decision: each env's smallest margin} over the discontinuous decisions the terms `names` read."""
    out = {}
    for dec, users in DISCONTINUOUS.items():
        if users and not set(users) & set(names):
            continue
        _, m, ex = ref["branches"][dec]
        m = np.where(ex, np.inf, m)
        out[dec] = m.reshape(m.shape[0], -1).min(axis=1) if m.size else np.full(m.shape[0], np.inf)
    return out


def coverage_problems(ref, par, only_positive):
    """What the coverage condition misses, from the reference's output alone ([] = all met)."""
    bad = []
    live = ~ref["reset"]
    for name in par["rows"]:
        if name == "termination" or (name == "collision" and not par["penalised"]):
            continue
        n = int((ref["terms"][name][0][live] != 0).sum())
        if n < 8:
            bad.append(f"term {name} non-zero in {n} non-reset envs")
    n = int(ref["terms"]["termination"][0].sum())
    if "termination" in par["rows"] and n < 2:
        bad.append(f"termination in {n} envs")
    for dec, (values, users) in BRANCHES.items():
        if (users and not set(users) & set(par["rows"])) or (dec == "collision" and not par["penalised"]):
            continue
        b = np.asarray(ref["branches"][dec][0])
        b = b.reshape(b.shape[0], -1)
        for v in values:
            n = int((b == v).any(axis=1).sum())
            if n < 2:
                bad.append(f"decision {dec}: branch {v} taken by {n} envs")
    for dec in ON_THRESHOLD:
        users = DISCONTINUOUS[dec]
        if users and not set(users) & set(par["rows"]):
            continue
        _, m, ex = ref["branches"][dec]
        n = int(((m == 0) & ex).reshape(m.shape[0], -1).any(axis=1).sum())
        if n < 2:
            bad.append(f"decision {dec}: {n} envs exactly on the threshold")
    if only_positive:
        neg = ref["pre_clip"] < 0
        if neg.sum() < 8 or (neg & (ref["terms"]["termination"][0] > 0)).sum() < 2:
            bad.append(f"negative pre-clip sum in {int(neg.sum())} envs, "
                       f"{int((neg & (ref['terms']['termination'][0] > 0)).sum())} of them terminating")
    return bad


# ---------------------------------------------------------------------------------- the state
def _random_row(g, par):
    """One env's state, every discontinuous decision away from its threshold by construction."""
    nb, nf, f32 = par["num_bodies"], len(par["feet"]), np.float32
    r = {}
    quat = g.normal(size=4) * [0.15, 0.15, 1.0, 0.0] + [0, 0, 0, 1.0]
    quat = (quat / np.linalg.norm(quat)).astype(f32)
    quat = (quat.astype(np.float64) / np.linalg.norm(quat.astype(np.float64))).astype(f32)
    root = np.zeros(13)
    root[:2] = g.uniform(-0.5, 0.5, 2)
    root[2] = g.uniform(0.2, 0.45)
    root[3:7] = quat
    root[7:13] = g.uniform(-1.0, 1.0, 6)
    r["root_states"] = root
    q = par["default_dof_pos"] + g.uniform(-0.3, 0.3, 12)
    q = np.clip(q, par["soft_lower"] + 0.01, par["soft_upper"] - 0.01)
    out = g.random(12) < 0.12
    side = g.random(12) < 0.5
    q = np.where(out, np.where(side, par["soft_lower"] - g.uniform(0.01, 0.2, 12), par["soft_upper"] + g.uniform(0.01, 0.2, 12)), q)
    r["dof_pos"] = q
    v = g.uniform(-2.5, 2.5, 12)
    over = g.random(12) < 0.15
    Lv = par["dof_vel_limits"] * par["soft_dof_vel_limit"]
    r["dof_vel"] = np.where(over, np.sign(v) * (Lv + g.uniform(0.05, 2.0, 12)), np.minimum(np.abs(v), 0.9 * Lv) * np.sign(v))
    t = g.uniform(-15.0, 15.0, 12)
    over = g.random(12) < 0.15
    Lt = par["torque_limits"] * par["soft_torque_limit"]
    r["torques"] = np.where(over, np.sign(t) * (Lt + g.uniform(0.05, 4.0, 12)), np.minimum(np.abs(t), 0.9 * Lt) * np.sign(t))
    cf = np.zeros((nb, 3))
    for b in par["penalised"]:
        if g.random() < 0.3:
            cf[b] = g.normal(size=3) * g.uniform(0.5, 3.0)
    in_contact = g.permutation(nf) < g.choice(nf + 1, p=_contact_count_p(nf))
    for i, b in enumerate(par["feet"]):
        kind = g.random()
        if in_contact[i]:
            cf[b] = [g.normal() * 2.0, g.normal() * 2.0, g.uniform(2.0, 40.0)]
            if kind < 0.25:   # a foot against a vertical surface
                cf[b, :2] = np.array([1.0, 0.3]) * 8.0 * cf[b, 2] * g.choice([-1, 1])
        elif kind < 0.2:      # a grazing contact: below the contact threshold, above no_fly's
            cf[b] = [g.normal() * 0.05, g.normal() * 0.05, g.uniform(0.3, 0.8)]
    r["contact_forces"] = cf
    r["actions"] = g.uniform(-1.5, 1.5, 12)
    r["last_actions"] = g.uniform(-0.5, 0.5, 12)
    r["last_dof_vel"] = g.uniform(-1.0, 1.0, 12)
    c = np.zeros(4)
    if g.random() < 0.3:
        c[:2] = g.uniform(-0.05, 0.05, 2)
    else:
        a, n = g.uniform(0, 2 * np.pi), g.uniform(0.2, 1.0)
        c[:2] = [n * np.cos(a), n * np.sin(a)]
    c[2] = g.uniform(-1, 1)
    c[3] = g.uniform(-3.14, 3.14)
    r["commands"] = c
    fat = np.where(g.random(4) < 0.3, 0.0, g.uniform(0.02, 0.9, 4))
    fat[nf:] = 0.0
    r["feet_air_time"] = fat
    return {k: np.asarray(x, f32) for k, x in r.items()}


def _contact_count_p(nf):
    p = np.ones(nf + 1)
    p[1] = 4.0   # exactly one foot down: no_fly's case
    return p / p.sum()


def build_state(par, seed, random_sums):
    """The deterministic N_ENVS-env state: random rows (redrawn until every discontinuous decision
    is MARGIN_MIN away from its threshold) and hand-placed rows with exact float32 values on both
    sides of every threshold.  Returns the state as float32 / int64 arrays keyed as the reference
    reads them, plus episode_sums [T, N]."""
    g = np.random.default_rng(seed)
    N, f32 = N_ENVS, np.float32
    L = int(par["max_episode_length"])
    interval = par["resample_interval"]
    feet, nf, dt = par["feet"], len(par["feet"]), f32(par["dt"])
    names = par["rows"]

    def ep_ok(ep):
        return (ep + 1) % interval != 0

    def one(g):   # a random row that no discontinuous decision is close to
        for _ in range(100):
            r = _random_row(g, par)
            s1 = {k: v[None] for k, v in r.items()}
            s1["episode_length"] = np.zeros(1, np.int64)
            rot = rotation_check(s1, par)
            dev = {k: v[0].astype(f32) for k, v in rot.items()}
            dev["measured_heights"] = np.zeros((1, 1), f32)
            ref = reference(s1, dev, dict(par, measure_heights=False))
            if min_margin(ref, slice(None), ALL_TERMS)[0] >= MARGIN_MIN:
                return r
        raise AssertionError("no random row with every decision margin >= MARGIN_MIN in 100 draws")

    rows = [one(g) for _ in range(N)]
    s = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    ep = g.integers(0, L - 2, N)
    while not ep_ok(ep).all():
        ep = np.where(ep_ok(ep), ep, g.integers(0, L - 2, N))
    for b in par["termination"]:
        s["contact_forces"][:, b] = 0.0

    # ---- hand-placed rows (each twice: rows 2i, 2i + 1), exact float32 values
    one_up = np.nextafter(f32(1.0), f32(2.0))
    tenth, tenth_up = f32(0.1), np.nextafter(f32(0.1), f32(1.0))
    grounded = ((0, 0, 8.0), None)
    foot_specs = [((0, 0, 1.0), 0.7), ((0, 0, one_up), 0.7), ((0, 0, 8.0), 0.0), ((0, 0, 8.0), dt),
                  ((0, 0, 8.0), 0.5), ((0, 0, 8.0), 0.7), ((5.0, 0, 1.0), 0.25), ((0, 0, 0), 0.25),
                  ((0, 0, 2.0), 0.0), ((0, 0, 4.0), 0.0)]
    foot_rows = [foot_specs[i:i + nf] for i in range(0, len(foot_specs), nf)]
    foot_rows = [fr + [grounded] * (nf - len(fr)) for fr in foot_rows]
    foot_rows += [[((6.0, 0, 1.0), None)] + [grounded] * (nf - 1), [((0, 6.0, -1.0), None)] + [grounded] * (nf - 1),
                  [((0, 0, tenth), None)] + [((0, 0, 0), None)] * (nf - 1),
                  [((0, 0, tenth_up), None)] + [((0, 0, 0), None)] * (nf - 1)]
    last = 2 * len(foot_rows) - 1      # the hand-placed rows are 0 .. max(last, 13), and the last two
    for i, fr in enumerate(foot_rows):
        for e in (2 * i, 2 * i + 1):
            for f, (F, t) in enumerate(fr):
                s["contact_forces"][e, feet[f]] = F
                if t is not None:
                    s["feet_air_time"][e, f] = t
    lo, hi = par["soft_lower"].astype(f32), par["soft_upper"].astype(f32)
    Lv = (par["dof_vel_limits"] * par["soft_dof_vel_limit"]).astype(f32)
    Lt = (par["torque_limits"].astype(f32) * f32(par["soft_torque_limit"])).astype(f32)   # the float32 product
    for e in (0, 1):
        s["dof_pos"][e, :4] = [lo[0], hi[1], lo[2] - f32(0.125), hi[3] + f32(0.125)]
        s["dof_vel"][e, :5] = [Lv[0] - f32(0.5), Lv[1], -(Lv[2] + f32(0.5)), Lv[3] + f32(1.0), -(Lv[4] + f32(3.0))]
        s["torques"][e, :3] = [Lt[0] - f32(1.0), -Lt[1], Lt[2] + f32(1.0)]
    pen = par["penalised"]
    air = 2 * -(-6 // nf)       # the rows of the six air-time specs: a moving command, so that the term is live
    s["commands"][:air, :2] = (0.25, -0.5)
    for e, c in ((air, (tenth, 0.0)), (air + 1, (0.0, -tenth)),    # the norm is float32(0.1) itself: neither < nor >
                 (air + 2, (0.0625, 0.0)), (air + 3, (0.0, 0.0625)), (air + 4, (0.0, -0.125)), (air + 5, (0.125, 0.0))):
        s["commands"][e, :2] = c
    if pen:
        for e, F in ((6, (0.0625, 0, 0)), (7, (0, 0, 0.0625)), (8, (0, 0.125, 0)), (9, (0, 0, -0.125))):
            s["contact_forces"][e, pen] = 0.0
            s["contact_forces"][e, pen[e % len(pen)]] = F
    tb = par["termination"]
    ep[[0, 1]] = L - 1          # the step makes it L: not yet a time-out
    ep[[N - 2, N - 1]] = L      # L + 1: a time-out
    for e in (10, 11):
        s["contact_forces"][e, tb[0]] = (0, 0, 1.0)     # not above 1
    for e in (12, 13):
        s["contact_forces"][e, tb[0]] = (0, 0, 2.0)
    # ---- resets among the random rows: contact terminations, pure time-outs, both
    free = list(range(max(last, 13) + 1, N - 2))
    for k, e in enumerate(free[:14]):
        if k < 7 or k >= 11:
            F = g.normal(size=3)
            s["contact_forces"][e, tb[k % len(tb)]] = (F / np.linalg.norm(F) * g.uniform(3.0, 10.0)).astype(f32)
        if k >= 7:
            ep[e] = L + int(g.integers(0, 3))
    assert ep_ok(ep).all(), "an env sits on a command-resample step"
    s["episode_length"] = ep.astype(np.int64)
    T = len(names)
    s["episode_sums"] = (g.uniform(-5.0, 5.0, (T, N)) if random_sums else np.zeros((T, N))).astype(f32)
    s["root_states"][:, :3] += par["env_origins"].astype(f32)
    return s


# ---------------------------------------------------------------------------------- the cases
def all_terms(cfg):
    for name, v in ALL_SCALES.items():
        setattr(cfg.rewards.scales, name, v)
    r = cfg.rewards
    r.soft_dof_pos_limit, r.soft_dof_vel_limit, r.soft_torque_limit = 0.9, 0.5, 0.8
    r.max_contact_force, r.base_height_target = 2.0, 0.3
    r.only_positive_rewards = False


def small(cfg):
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.max_init_terrain_level = 3, 2, 2


def _case(task, all_on, clip=False, sums=True, oracle=True):
    def overrides(cfg):
        small(cfg)
        if all_on:
            all_terms(cfg)
            cfg.rewards.only_positive_rewards = clip
        else:
            cfg.rewards.max_contact_force = 2.0
    return dict(task=task, overrides=overrides, all_on=all_on, clip=clip, random_sums=sums, oracle=oracle)


# oracle=False: the CPU oracle backend has no privileged row and no history, the HIP kernels' own
# instantiations for them run on the GPU only
CASES = {
    "flat_all_terms": _case("go1_flat_bench", True, sums=False),
    "flat_all_terms_positive_clip": _case("go1_flat_bench", True, clip=True),
    "rough_all_terms": _case("go1_rough", True),
    "rough_asym_all_terms": _case("go1_rough_asym", True, oracle=False),
    "rough_hist_all_terms": _case("go1_rough_hist", True, oracle=False),
    "cassie_shipped": _case("cassie", False),
}


# ---------------------------------------------------------------------------------- the test body
STATE_FIELDS = {"root_states": "root_states", "dof_pos": "dof_pos", "dof_vel": "dof_vel", "torques": "torques",
                "contact_forces": "contact_forces", "actions": "actions", "last_actions": "last_actions",
                "last_dof_vel": "last_dof_vel", "commands": "commands", "feet_air_time": "_feet_air_time_full",
                "episode_length": "_episode_length_buf", "episode_sums": "_episode_sums_buf"}


def load_state(env, s):
    import torch
    for key, attr in STATE_FIELDS.items():
        t = getattr(env, attr)
        t.copy_(torch.from_numpy(np.ascontiguousarray(s[key])).to(t.device))


def _np(t):
    return t.detach().cpu().numpy().copy()


def capture_state(env):
    """The state as load_state writes it, read from an env (before its step)."""
    return {key: _np(getattr(env, attr)) for key, attr in STATE_FIELDS.items()}


def worst_ratio(err, bound):
    """max err / bound; an error where the bound is 0 is infinitely over it."""
    err, bound = np.broadcast_arrays(_f(err), _f(bound))
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def check_post_physics(env, s, random_sums, fused=False):
    """One post_physics_step of `env` from state `s` against the reference (compare_with_reference)."""
    import torch
    load_state(env, s)
    env.common_step_counter = 7
    env.post_physics_step(fused=True) if fused else env.post_physics_step()
    if str(env.device).startswith("cuda"):
        torch.cuda.synchronize()
    return compare_with_reference(env, s, random_sums)


def compare_with_reference(env, s, random_sums=True, sums_only=False):
    """What `env` holds after one post_physics_step from state `s`, against the reference.  Returns
    the worst error-to-bound ratio per compared quantity; raises AssertionError listing every
    quantity over its bound, with its ratio.  sums_only: the rotated vectors and the episode-sum rows
    of the non-reset envs alone, on a state the builder did not make - envs on a command-resample
    step (a Philox draw enters) or within MARGIN_MIN of a threshold are left to the caller."""
    par = params_from_env(env)
    dev = {k: _np(getattr(env, k)) for k in ("measured_heights", "base_lin_vel", "base_ang_vel", "projected_gravity")}
    ratios, failures = {}, []

    def compare(name, got, want, bound):
        ratios[name] = worst_ratio(np.abs(_f(got) - _f(want)), bound)
        if not ratios[name] <= 1.0:
            failures.append(f"{name}: error / bound = {ratios[name]:.3g}")

    for name, (want, bound) in rotation_check(s, par).items():
        compare(name, dev[name], want, bound)
    ref = reference(s, dev, par)
    if not sums_only:
        # the conditions on the inputs, from the reference's output alone, before any comparison is judged
        m, dec = min_margin(ref, slice(None), par["rows"])
        assert m >= MARGIN_MIN, f"decision {dec} is {m:.3g} from its threshold"
        n_reset = int(ref["reset"].sum())
        assert 0.2 * N_ENVS <= n_reset <= 0.3 * N_ENVS, f"{n_reset} of {N_ENVS} envs reset"
        bad = coverage_problems(ref, par, par["only_positive"])
        assert not bad, "coverage condition not met:\n  " + "\n  ".join(bad)

    live, reset = ~ref["reset"], ref["reset"]
    if sums_only:
        live = live & ((np.asarray(s["episode_length"]) + 1) % par["resample_interval"] != 0)
        for m in env_margins(ref, par["rows"]).values():
            live = live & (m >= MARGIN_MIN)
        ratios["envs"] = int(live.sum())
    sums, start = _f(_np(env._episode_sums_buf)), _f(s["episode_sums"])
    R = int(reset.sum())
    extras = _f(_np(env._extras_buf))
    for t, name in enumerate(par["rows"]):
        want = start[t] + ref["prod"][name]
        bound = ref["prod_bound"][name] + U * (np.abs(want) + ref["prod_bound"][name])
        compare(f"sum[{name}]", sums[t][live], want[live], bound[live])                       # 1
        if not sums_only:
            if name in EXACT_TERMS and not random_sums:
                exact = (_f(ref["terms"][name][0]).astype(np.float32) * np.float32(par["scales"][name])).astype(np.float64)
                if not np.array_equal(sums[t][live], exact[live]):
                    failures.append(f"sum[{name}]: not the exact float32 product in {int((sums[t][live] != exact[live]).sum())} envs")
            if sums[t][reset].any():
                failures.append(f"sum[{name}]: not zeroed on reset")                           # 2
            if R:
                den = R * par["max_episode_length_s"]
                compare(f"extras[{name}]", extras[t], want[reset].sum() / den,
                        (bound[reset].sum() + C_nk(R, 1) * U * np.abs(want[reset]).sum()) / den)
    if sums_only:
        assert not failures, "\n".join(failures)
        return ratios
    T = len(par["rows"])
    if R:
        if extras[T + 1] != R:
            failures.append(f"extras reset count {extras[T + 1]} != {R}")
        if env.cfg.terrain.curriculum:   # the mean of the levels the step left (the curriculum itself: the oracle's)
            lv = _f(_np(env.terrain_levels))
            compare("extras[terrain_level]", extras[T], lv.mean(), 2 * U * lv.mean())
        episode = env.extras["episode"]
        for key, row in env._extras_rows:
            if float(episode[key]) != np.float32(extras[row]):
                failures.append(f"extras['episode'][{key!r}] is not row {row} of the extras buffer")
        if set(episode) != {k for k, _ in env._extras_rows}:
            failures.append(f"extras['episode'] keys {sorted(episode)}")
    compare("rew_buf", _np(env.rew_buf), ref["rew"], ref["rew_bound"])                         # 3
    for name, got, want in (("reset_buf", env.reset_buf, ref["reset"]), ("time_out_buf", env.time_out_buf, ref["time_out"]),
                            ("_extras_time_outs", env._extras_time_outs, ref["time_out"]),
                            ("_episode_length_buf", env._episode_length_buf, ref["episode_length"])):   # 4
        if not np.array_equal(_np(got).astype(np.int64), np.asarray(want).astype(np.int64)):
            failures.append(f"{name}: differs in envs {np.nonzero(_np(got).astype(np.int64) != np.asarray(want).astype(np.int64))[0][:8]}")
    nf = len(par["feet"])
    fat = ref["feet_air_time"][:, :nf]
    compare("feet_air_time", _np(env.feet_air_time), fat, 2 * U * np.abs(fat))                 # 5
    assert not failures, "\n".join(failures)
    return ratios


def run_case(name, device="cpu", backend="oracle"):
    from oracle_backend import make_env
    case = CASES[name]
    env = make_env(case["task"], num_envs=N_ENVS, device=device, backend=backend, overrides=case["overrides"])
    par = params_from_env(env)
    if case["all_on"]:
        assert sorted(par["rows"]) == sorted(ALL_SCALES)
        assert len(par["rows"]) + 2 == MAX_TERMS, "the all-terms cases fill the extras finalize's row loop: T + 2 = 24"
    s = build_state(par, seed=2024, random_sums=case["random_sums"])
    ratios = check_post_physics(env, s, case["random_sums"], fused=backend != "oracle")
    print(name, backend, {k: round(v, 3) for k, v in ratios.items()})
    return ratios
