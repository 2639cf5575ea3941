"""Left-right mirror tables of the rows PPO trains on (rsl_rl 2.x symmetry_cfg.use_data_augmentation).

The mirror is the reflection across the robot's x-z plane.  Every kind of row gets a signed
permutation `(perm, sign)`: `mirror(x)[c] = sign[c] * x[perm[c]]`.  A polar vector
(velocity, gravity, force) mirrors as (+, -, +); an angular quantity is a pseudo-vector and mirrors
as (-, +, -).  A joint's partner is the same joint of the other side's leg, found by explicit name
prefixes (no fixed leg order: ANYmal's dofs run LF, LH, RF, RH); its sign follows from the model's
joint axes in the base frame at the zero pose: sign[j] = a[partner(j)] . diag(-1, 1, -1) a[j].

Pure Python (no torch, no library): this module is the one place that knows the rows' mirror
arithmetic.  `apply` mirrors anything indexable by a list (numpy arrays, torch tensors) on its last axis
given index / sign arrays of the caller's own kind.
"""

# left/right leg-name prefixes of the quadrupeds here, one family per naming scheme
PREFIX_PAIRS = ((("FL", "FR"), ("RL", "RR")),      # Go1 / A1 / Aliengo
                (("LF", "RF"), ("LH", "RH")))      # ANYmal-B / C
PROPRIO = 48            # base lin vel, ang vel, gravity, commands, dof pos, dof vel, actions
POLAR = (1.0, -1.0, 1.0)
AXIAL = (-1.0, 1.0, -1.0)
SIGN_TOL = 1e-6


def _prefix(name):
    return name.split("_")[0]


def leg_pairs(names):
    """The prefix family (two (left, right) pairs) whose four prefixes all occur in `names`;
    ValueError naming the missing pairs of every family otherwise (Cassie, an arm, ...)."""
    have = {_prefix(n) for n in names}
    missing = []
    for family in PREFIX_PAIRS:
        miss = [f"{l}<->{r}" for l, r in family if l not in have or r not in have]
        if not miss:
            return family
        missing.append(" and ".join(miss))
    raise ValueError("symmetry: the model has no left/right leg pairs to mirror (missing " + ", or ".join(missing) +
                     f" among {sorted(have)})")


def partners(names, family):
    """perm over `names`: the same name with the other side's prefix; names without a leg prefix
    (the base) map to themselves.  ValueError for a name whose partner is absent."""
    other = {}
    for l, r in family:
        other[l], other[r] = r, l
    index = {n: i for i, n in enumerate(names)}
    perm = []
    for n in names:
        p = _prefix(n)
        if p not in other:
            perm.append(index[n])
            continue
        twin = other[p] + n[len(p):]
        if twin not in index:
            raise ValueError(f"symmetry: {n!r} has no mirror partner {twin!r}")
        perm.append(index[twin])
    return perm


def _matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def joint_axes_in_base(joints, leg_dof):
    """Each joint's axis in the base frame at the zero pose: the legs are chains of `leg_dof` joints
    off the base, joint frame = parent frame x the joint's `rot` (row-major 3x3)."""
    out, R = [], None
    for j, jt in enumerate(joints):
        rot = [list(jt["rot"][3 * i:3 * i + 3]) for i in range(3)]
        R = rot if j % leg_dof == 0 else _matmul(R, rot)
        out.append([sum(R[i][k] * jt["axis"][k] for k in range(3)) for i in range(3)])
    return out


def joint_table(dof_names, joints, leg_dof, default_dof_pos=None):
    """(perm, sign) of a per-joint row (dof positions / velocities / actions / torques).
    default_dof_pos: observations hold q - q0 and actions are offsets from q0, so q0 must itself be
    mirror-symmetric (q0[partner(j)] == sign[j] * q0[j]); ValueError otherwise."""
    perm = partners(dof_names, leg_pairs(dof_names))
    axes = joint_axes_in_base(joints, leg_dof)
    sign = []
    for j, p in enumerate(perm):
        s = sum(axes[p][i] * AXIAL[i] * axes[j][i] for i in range(3))
        if abs(abs(s) - 1.0) > SIGN_TOL:
            raise ValueError(f"symmetry: the axes of {dof_names[j]} and {dof_names[p]} are not mirror images "
                             f"(sign {s:.6f}, not +-1)")
        sign.append(1.0 if s > 0 else -1.0)
    if default_dof_pos is not None:
        q0 = [float(v) for v in default_dof_pos]
        for j, p in enumerate(perm):
            if abs(q0[p] - sign[j] * q0[j]) > SIGN_TOL:
                raise ValueError(f"symmetry: default_joint_angles are not mirror-symmetric: {dof_names[p]} = {q0[p]} "
                                 f"but {dof_names[j]} = {q0[j]} mirrors to {sign[j] * q0[j]}")
    return perm, sign


def height_table(points_x, points_y):
    """perm of the height scan, `meshgrid(x, y, indexing="ij")` flattened: point ix * ny + iy maps to
    the point of the same x whose y is negated.  ValueError for y values not symmetric about 0."""
    ys = [float(v) for v in points_y]
    ny = len(ys)
    twin = []
    for y in ys:
        hits = [k for k, v in enumerate(ys) if abs(v + y) <= SIGN_TOL]
        if len(hits) != 1:
            raise ValueError(f"symmetry: terrain.measured_points_y is not symmetric about 0 (no unique point at "
                             f"y = {-y} for the one at y = {y})")
        twin.append(hits[0])
    return [ix * ny + twin[iy] for ix in range(len(points_x)) for iy in range(ny)]


def _shift(table, off):
    return [p + off for p in table[0]], list(table[1])


def _concat(*tables):
    perm, sign = [], []
    for p, s in tables:
        perm += p
        sign += s
    return perm, sign


def _triple(signs, off):
    return [off, off + 1, off + 2], list(signs)


def base_table(num_obs, joint, points_x=(), points_y=()):
    """(perm, sign) of the `compute_observations` row (layout as `_get_noise_scale_vec`): lin vel,
    ang vel, gravity, commands (vx, vy, yaw rate), dof pos, dof vel, actions, height scan."""
    n = len(joint[0])
    parts = [_triple(POLAR, 0), _triple(AXIAL, 3), _triple(POLAR, 6), _triple((1.0, -1.0, -1.0), 9)]
    parts += [_shift(joint, 12 + k * n) for k in range(3)]
    width = 12 + 3 * n
    if num_obs > width:
        hp = height_table(points_x, points_y)
        parts.append(([width + p for p in hp], [1.0] * len(hp)))
        width += len(hp)
    if width != num_obs:
        raise ValueError(f"symmetry: an observation row of {num_obs} entries is not {12 + 3 * n} proprioceptive "
                         f"entries + {len(points_x) * len(points_y)} height points")
    return _concat(*parts)


def privileged_table(base, layout, joint, dyn_perm, feet_perm):
    """(perm, sign) of the privileged row `[clean | tail]` (envs/base/privileged.py): `clean` through
    the base table; friction and base_mass unchanged, mass_scale with left/right bodies swapped
    (dyn_perm), feet_contact with the feet swapped (feet_perm), feet_forces likewise with the
    components (+, -, +), torques through the joint table."""
    parts = [base]
    for name, _, sl in layout.terms:
        w = sl.stop - sl.start
        if name in ("friction", "base_mass"):
            t = (list(range(w)), [1.0] * w)
        elif name == "mass_scale":
            t = (list(dyn_perm), [1.0] * w)
        elif name == "feet_contact":
            t = (list(feet_perm), [1.0] * w)
        elif name == "feet_forces":
            t = ([3 * f + i for f in feet_perm for i in range(3)], list(POLAR) * len(feet_perm))
        elif name == "torques":
            t = (list(joint[0]), list(joint[1]))
        else:
            raise ValueError(f"symmetry: no mirror rule for the privileged term {name!r}")
        if len(t[0]) != w:
            raise ValueError(f"symmetry: privileged term {name!r} is {w} wide, its mirror table {len(t[0])}")
        parts.append(_shift(t, sl.start))
    return _concat(*parts)


def history_table(base, layout):
    """(perm, sign) of the history row `[obs | frame_1 .. frame_H]` (envs/base/history.py): each frame
    through the first frame_width entries of the base table, shifted to the frame's columns.
    ValueError for a frame_width whose prefix the permutation leaves (one that cuts a joint block)."""
    w = layout.frame_width
    head = (base[0][:w], base[1][:w])
    if any(p >= w for p in head[0]):
        raise ValueError(f"symmetry: history.frame_width = {w} cuts through a block the mirror permutes (column "
                         f"{next(c for c, p in enumerate(head[0]) if p >= w)} mirrors from column "
                         f"{next(p for p in head[0] if p >= w)})")
    return _concat(base, *[_shift(head, layout.frame(k).start) for k in range(1, layout.frames + 1)])


def check(table):
    """A table must be an involution: perm[perm] == arange and sign * sign[perm] == 1."""
    perm, sign = table
    for c, p in enumerate(perm):
        if not 0 <= p < len(perm) or perm[p] != c or sign[c] * sign[p] != 1.0:
            raise ValueError(f"symmetry: the mirror table is not an involution at column {c}")
    return table


def apply(x, perm, sign):
    """mirror(x) on the last axis: sign * x[..., perm] (perm / sign of x's own array kind)."""
    return x[..., perm] * sign


def env_tables(asset_data, dof_names, dyn_names, feet_names, default_dof_pos, num_base_obs, points_x, points_y,
               privileged_layout=None, history_layout=None):
    """Every table of one env as Python lists: {"actions", "obs", "critic_obs" (None without a
    privileged row)}, each checked to be an involution."""
    joint = joint_table(dof_names, asset_data["joints"], int(asset_data.get("leg_dof", 3)), default_dof_pos)
    family = leg_pairs(dof_names)
    base = base_table(num_base_obs, joint, points_x, points_y)
    obs = base if history_layout is None else history_table(base, history_layout)
    critic = None
    if privileged_layout is not None:
        critic = privileged_table(base, privileged_layout, joint, partners(dyn_names, family),
                                  partners(feet_names, family))
    return {"actions": check(joint), "obs": check(obs), "critic_obs": check(critic) if critic is not None else None}
