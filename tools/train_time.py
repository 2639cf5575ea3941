"""Wall time per training iteration of OnPolicyRunner.learn as scripts/train.py runs it (with a log
directory) and as bench.py runs it (without): go1_rough (or --task), 4096 envs.

    python tools/train_time.py [--configs logged,logged_old,logged_defer,unlogged] [--iters 50]
                               [--warmup 10] [--windows 5] [--task go1_rough]
                               [--no_fused_update] [--teacher CHECKPOINT]

Configurations (one runner with a temporary log directory, one without, on one env):
    logged        log directory, device episode statistics (the default path)
    logged_old    log directory, LGX_DEVICE_STATS=0 (rsl_rl's torch / deque block)
    logged_defer  log directory, LGX_DEFER_LOG=1
    unlogged      no log directory
A window is one learn(iters) between two device synchronisations, its stdout discarded; with a
log directory it contains the checkpoints learn() writes (every save_interval iterations and at
its end).  The windows of the configurations alternate, after learn(warmup) of each.  Prints one
JSON line: per configuration the median ms per iteration and every window's, the last iteration's
collection / learn phases, and for a task with symmetry augmentation (go1_rough_sym) the augment
launch's time from HIP events around it.
--no_fused_update times the autograd update (algorithm.use_fused_update = False); a Distillation task
(go1_rough_distill) takes its teacher from --teacher or keeps a randomly initialised one.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import legged_gym_amd.envs  # noqa: E402,F401
from legged_gym_amd.utils.helpers import get_args  # noqa: E402
from legged_gym_amd.utils.task_registry import task_registry  # noqa: E402

ENV = {"logged": {}, "logged_old": {"LGX_DEVICE_STATS": "0"}, "logged_defer": {"LGX_DEFER_LOG": "1"}, "unlogged": {}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="logged,logged_old,logged_defer,unlogged")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--task", default="go1_rough")
    ap.add_argument("--no_fused_update", action="store_true",
                    help="algorithm.use_fused_update = False: the autograd update (the fused update's yardstick)")
    ap.add_argument("--teacher", default=None,
                    help="Distillation tasks: a go1_rough_teacher checkpoint; without one the teacher keeps its "
                         "random initial weights (the time per iteration does not depend on them)")
    a = ap.parse_args()
    configs = a.configs.split(",")
    assert all(c in ENV for c in configs), f"configurations: {sorted(ENV)}"
    assert torch.cuda.is_available(), "train_time.py measures on the GPU"
    task = a.task
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg.env.num_envs = a.num_envs
    if a.no_fused_update:
        train_cfg.algorithm.use_fused_update = False
    cli = get_args(["--sim_device", "cuda:0", "--rl_device", "cuda:0", "--headless", "--task", task])
    out = {c: [] for c in configs}
    with tempfile.TemporaryDirectory() as tmp, open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
        env, _ = task_registry.make_env(task, args=cli, env_cfg=env_cfg)
        runners = {}
        for logged in sorted({c != "unlogged" for c in configs}):
            runners[logged], _ = task_registry.make_alg_runner(env, name=task, args=cli, train_cfg=train_cfg,
                                                               log_root=tmp if logged else None)

        for r in runners.values():   # Distillation: a teacher (its values do not matter to the clock)
            if hasattr(r.alg.actor_critic, "loaded_teacher"):
                if a.teacher:
                    r.load(a.teacher)
                r.alg.actor_critic.loaded_teacher = True

        # symmetry augmentation (algorithm.symmetry): HIP events around each update's augment launch
        fused = [r.alg._fused for r in runners.values()
                 if getattr(r.alg, "_fused", None) is not None and getattr(r.alg.storage, "symmetry", None) is not None]
        for f in fused:
            f.time_augment = True

        def learn(config, n):
            for k in ("LGX_DEVICE_STATS", "LGX_DEFER_LOG"):
                os.environ.pop(k, None)
            os.environ.update(ENV[config])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runners[config != "unlogged"].learn(n)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for c in configs:
            learn(c, a.warmup)
        for _ in range(a.windows):
            for c in configs:
                out[c].append(round(learn(c, a.iters), 4))
        # the last iteration's phases (the runner's stream events) and every augment launch's time
        phases = {("logged" if logged else "unlogged"): {k: round(r.last_iteration_stats[k] * 1e3, 4)
                                                         for k in ("collection_time", "learn_time")}
                  for logged, r in runners.items()}
        augment = [e0.elapsed_time(e1) * 1e3 for f in fused for e0, e1 in f.augment_events]
    res = {"task": task, "num_envs": a.num_envs, "fused_update": not a.no_fused_update, "iters_per_window": a.iters, "warmup_iters": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "ms_per_iteration": {c: {"median": round(statistics.median(w), 4), "windows": w} for c, w in out.items()},
           "last_iteration_phases_ms": phases}
    if augment:
        res["augment_us"] = {"median": round(statistics.median(augment), 2), "launches": len(augment)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
