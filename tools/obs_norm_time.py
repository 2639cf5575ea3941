"""Device time of the observation normaliser's two launches (csrc/lgx_obsnorm.hip) from stream events.

    python tools/obs_norm_time.py [--num_envs 4096] [--widths 235,253] [--launches 200] [--windows 5]

A window is `launches` back-to-back launches between two events, enqueued while a long matmul still
occupies the stream, so the interval holds device time only (kernels and the gaps between their
dispatches), not the host's enqueue rate.  Both normalisers ride in each launch, as in the runner.
Prints one JSON line: microseconds per launch for the partials launch, the merge-and-apply launch
(update on), the frozen apply, and the pair as a training step issues it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from legged_gym_amd.rl.normalizer import EmpiricalNormalization, rows_per_part  # noqa: E402
from legged_gym_amd.sim import abi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--widths", default="235,253")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "obs_norm_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    widths = [int(w) for w in a.widths.split(",")]
    N, P = a.num_envs, -(-a.num_envs // rows_per_part())
    norms = [EmpiricalNormalization(w, device=dev) for w in widths]
    lib = norms[0]._lib
    xs = [torch.randn(N, w, device=dev) for w in widths]
    ys = [torch.empty_like(x) for x in xs]
    parts = [torch.empty(P, 1 + 2 * w, dtype=torch.float64, device=dev) for w in widths]
    states = [[torch.zeros(1 + 2 * w, dtype=torch.float64, device=dev) for _ in range(2)] for w in widths]

    def jobs(update, flip=0):
        js = (abi.LgxObsNormJob * len(widths))()
        for j, w, x, y, p, s in zip(js, widths, xs, ys, parts, states):
            j.x, j.y, j.rows, j.width, j.update, j.eps = x.data_ptr(), y.data_ptr(), N, w, update, 1e-2
            j.parts, j.nparts, j.state_in, j.state_out = p.data_ptr(), P, s[flip].data_ptr(), s[flip ^ 1].data_ptr()
        return js
    train, frozen = [jobs(1, 0), jobs(1, 1)], jobs(0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = len(widths)
    kinds = {
        "partials": lambda k: lib.lgx_obs_norm_partials(train[0], n, stream),
        "merge_apply": lambda k: lib.lgx_obs_norm_apply(train[k & 1], n, stream),
        "frozen_apply": lambda k: lib.lgx_obs_norm_apply(frozen, n, stream),
        "partials_then_merge_apply": lambda k: lib.lgx_obs_norm_partials(train[0], n, stream)
        or lib.lgx_obs_norm_apply(train[k & 1], n, stream),
    }
    big = torch.randn(8192, 8192, device=dev)
    out = {}
    for name, launch in kinds.items():
        windows = []
        for w in range(a.windows + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):
                big @ big                      # keeps the stream busy while the launches are enqueued
            e0.record()
            for k in range(a.launches):
                assert launch(k) == 0, lib.lgx_last_error()
            e1.record()
            e1.synchronize()
            if w:                              # (window 0 warms up)
                windows.append(round(e0.elapsed_time(e1) * 1e3 / a.launches, 3))
        out[name] = {"median_us": statistics.median(windows), "windows_us": windows}
    print(json.dumps({"num_envs": N, "widths": widths, "rows_per_part": rows_per_part(), "partials": P,
                      "launches_per_window": a.launches, "device": torch.cuda.get_device_name(0),
                      "us_per_launch": out}), flush=True)


if __name__ == "__main__":
    main()
