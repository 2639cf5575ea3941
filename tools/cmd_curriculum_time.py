"""Device time of the command curriculum's launches (csrc/lgx_cmd_curriculum.hip) from stream events.

    python tools/cmd_curriculum_time.py [--task go1_rough] [--num_envs 4096] [--launches 100] [--windows 5]

A window is `launches` back-to-back env.post_physics_step() calls between two events, enqueued while
long matmuls still occupy the stream, so the interval holds device time only.  The same window is
taken on steps that are no curriculum steps and on curriculum steps; the difference per launch is
what a curriculum step adds: the decide + patch pair and the clone of max_command_x.  Two cases:
  idle    nothing resets or the tracking is poor: decide finds no change, patch returns at once
  widen   every env resets with good tracking and the range moves: decide writes it, patch redraws
          every env's command.  Each launch of these windows (both kinds of step) is preceded by
          the fills that script the state and by lgx_set_command_range, which puts the range back.
Prints one JSON line (microseconds per launch).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="go1_rough")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cmd_curriculum_time.py measures on the GPU"
    import legged_gym_amd.envs  # noqa: F401
    from legged_gym_amd.utils.helpers import get_args
    from legged_gym_amd.utils.task_registry import task_registry
    cfg = type(task_registry.get_cfgs(a.task)[0])()
    cfg.env.num_envs = a.num_envs
    cfg.seed = 1
    cfg.commands.curriculum = True
    cfg.commands.ranges.lin_vel_x = [-0.5, 0.5]
    env, _ = task_registry.make_env(a.task, args=get_args(["--sim_device", "cuda:0", "--headless"]), env_cfg=cfg)
    env.reset()
    L = int(env.max_episode_length)
    big = torch.randn(8192, 8192, device="cuda:0")
    sums = env.episode_sums["tracking_lin_vel"]
    perfect = float(env.reward_scales["tracking_lin_vel"]) * L     # the scale holds dt: reward 1 on every step

    def window(curriculum, widen):
        for _ in range(3):
            big @ big
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            if widen:
                env.episode_length_buf.fill_(L)     # every env times out ...
                sums.fill_(perfect)                 # ... after an episode of perfect tracking
                env.set_command_range("lin_vel_x", -0.5, 0.5)
            env.common_step_counter = L - 1 if curriculum else L
            env.post_physics_step(fused=True)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches

    out = {"task": a.task, "num_envs": a.num_envs, "max_episode_length": L, "launches": a.launches, "windows": a.windows}
    for case, widen in (("idle", False), ("widen", True)):
        window(True, widen), window(False, widen)       # warm-up
        cur = [window(True, widen) for _ in range(a.windows)]
        base = [window(False, widen) for _ in range(a.windows)]
        out[case] = {"curriculum_step_us": round(statistics.median(cur), 2),
                     "other_step_us": round(statistics.median(base), 2),
                     "added_us": round(statistics.median(cur) - statistics.median(base), 2),
                     "curriculum_step_us_all": [round(v, 2) for v in cur],
                     "other_step_us_all": [round(v, 2) for v in base]}
        if widen:
            out[case]["widenings"] = int(env.command_curriculum_state[2].item())
    out["added_us_per_step_amortised"] = {k: round(out[k]["added_us"] / L, 4) for k in ("idle", "widen")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
