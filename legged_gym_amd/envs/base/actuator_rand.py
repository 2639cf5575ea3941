"""Per-env actuator randomisation: the tables the physics launch reads (lgx_bind_actuator_rand).

The reference randomises friction, masses and pushes; everything about its actuator is one value
for all envs, so there are no reference semantics to follow: the tables are this project's own
(DESIGN.md §4.1b).  Per env e and joint j the drive's gains are kp * kp_scale[e, j] and
kd * kd_scale[e, j]; motor strength is no table of its own, it multiplies both scales.  lag[e] is the
number of substeps an action waits before it reaches the joints of env e (control.decimation = one
whole control step).

`draw` is a pure function of (config, sizes, seed): uniform draws per env and joint, taken once at
creation as friction and masses are, from a torch.Generator of its own - no other draw of the env
changes order or value when a flag here is switched.
"""
import torch

SEED_SALT = 0x61637472616E64   # "actrand": the tables' stream is not the env seed's own


def _range(name, rng):
    lo, hi = rng
    if lo > hi:
        raise ValueError(f"actuator_rand.{name} = [{lo}, {hi}]: the lower bound is above the upper")
    return lo, hi


def _scale_range(name, rng):
    lo, hi = _range(name, rng)
    if lo <= 0:
        raise ValueError(f"actuator_rand.{name} = [{lo}, {hi}]: a gain scale must be > 0")
    return float(lo), float(hi)


def draw(cfg, num_envs, num_dof, decimation, seed, device="cpu"):
    """(kp_scale, kd_scale, lag) for `cfg` (a LeggedRobotCfg.actuator_rand, or None: all off):
    kp_scale / kd_scale float32 [num_envs, num_dof] = strength * factor (products in float32), None
    unless randomize_motor_strength or the factor's own flag is set; lag int32 [num_envs], inclusive
    integers of lag_substeps_range, None unless randomize_lag.  The four streams are drawn in a fixed
    order whatever the flags, so one flag never moves another's values.  ValueError for a range with
    lo > hi, a scale <= 0, or a lag outside [0, decimation]."""
    flag = lambda n: bool(getattr(cfg, n, False))
    strength_on, kp_on, kd_on, lag_on = (flag("randomize_motor_strength"), flag("randomize_kp"), flag("randomize_kd"),
                                         flag("randomize_lag"))
    if not (strength_on or kp_on or kd_on or lag_on):
        return None, None, None
    ranges = {}
    for on, name in ((strength_on, "motor_strength_range"), (kp_on, "kp_factor_range"), (kd_on, "kd_factor_range")):
        ranges[name] = _scale_range(name, getattr(cfg, name)) if on else (1.0, 1.0)
    lag_lo, lag_hi = 0, 0
    if lag_on:
        lag_lo, lag_hi = _range("lag_substeps_range", cfg.lag_substeps_range)
        if lag_lo != int(lag_lo) or lag_hi != int(lag_hi):
            raise ValueError(f"actuator_rand.lag_substeps_range = [{lag_lo}, {lag_hi}]: whole substeps")
        lag_lo, lag_hi = int(lag_lo), int(lag_hi)
        if lag_lo < 0 or lag_hi > decimation:
            raise ValueError(f"actuator_rand.lag_substeps_range = [{lag_lo}, {lag_hi}] leaves [0, control.decimation"
                             f" = {decimation}]")
    gen = torch.Generator(device="cpu").manual_seed((int(seed) ^ SEED_SALT) & 0x7FFFFFFFFFFFFFFF)

    def uniform(name):
        lo, hi = ranges[name]
        u = torch.rand(num_envs, num_dof, generator=gen, dtype=torch.float32)
        return (torch.tensor(lo, dtype=torch.float32) + torch.tensor(hi - lo, dtype=torch.float32) * u).clamp_(lo, hi)

    strength, kp_factor, kd_factor = (uniform("motor_strength_range"), uniform("kp_factor_range"),
                                      uniform("kd_factor_range"))
    lag = torch.randint(lag_lo, lag_hi + 1, (num_envs,), generator=gen, dtype=torch.int32)
    kp_scale = (strength * kp_factor).to(device).contiguous() if strength_on or kp_on else None
    kd_scale = (strength * kd_factor).to(device).contiguous() if strength_on or kd_on else None
    return kp_scale, kd_scale, lag.to(device).contiguous() if lag_on else None
