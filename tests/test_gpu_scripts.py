"""GPU: the train / play entry points end to end (legged_gym/scripts/train.py, play.py):
2 PPO iterations with checkpointing on the HIP path, then resume the latest checkpoint,
export the actor as TorchScript and run the policy."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_train_then_play(gpu, tmp_path):
    from legged_gym_amd import LEGGED_GYM_ROOT_DIR
    from legged_gym_amd.scripts.play import play
    from legged_gym_amd.scripts.train import train
    from legged_gym_amd.utils import get_args
    exp = f"pytest_{os.getpid()}"
    common = ["--task", "go1", "--headless", "--num_envs", "64", "--experiment_name", exp]
    train(get_args(common + ["--max_iterations", "2"]))
    root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp)
    runs = os.listdir(root)
    assert len(runs) == 1 and "model_2.pt" in os.listdir(os.path.join(root, runs[0]))
    # go1_config.py pins load_run to the authors' run; point it at ours
    finished = play(get_args(common + ["--load_run", runs[0]]), steps=60)
    assert os.path.exists(os.path.join(root, "exported", "policies", "policy_1.pt"))
    pol = torch.jit.load(os.path.join(root, "exported", "policies", "policy_1.pt"))
    assert pol(torch.zeros(1, 48)).shape == (1, 12)


def test_bench_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    """A plain `bench.py --steps K --warmup W` prints the headline line alone (the kernel timings,
    rooflines and CPU baseline belong to --full), K sets the timed iterations, and --dump-outputs
    writes the last iteration's results as float32 / float64 .npy files of at most 64 MB."""
    import json
    import subprocess
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--task", "go1_flat_bench", "--num_envs", "300", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "fp32" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(24 * 300 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert d["full"] is False
    assert not {"roofline", "lgx_kernels", "cpu_baseline", "iteration_roofline"} & set(d)
    files = sorted(os.listdir(out))
    assert {"policy_params.npy", "obs.npy", "storage_actions.npy", "storage_returns.npy", "update_stats.npy"} <= set(files)
    arrays = {f: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["obs.npy"].shape == (300, 48)
    assert arrays["storage_actions.npy"].shape == (24, 256, 12)   # the seeded sample of 256 envs
    assert np.abs(arrays["storage_actions.npy"]).max() > 0 and np.abs(arrays["policy_params.npy"]).max() > 0
