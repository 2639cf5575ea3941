"""The physics kernel's corrected-trimesh queue at a bench size, in the state of tools/phys_bench.py
(30 env steps of seeded random actions after reset).

  forms [task] [num_envs] [reps] [launches]
      one env per LGX_TM_STAGE2 value (rows, lane, packed, unset) in this process, all in the same
      state (the forms give the same bits); the physics launch of each is timed with HIP events,
      the forms alternated `reps` times.  Prints one JSON line.
  hist [task] [num_envs] [out.json]
      needs a tuning build (tools/phase_clock.sh with CLK_EXTRA=-DLGX_PHASE_CLOCK_BUF, selected by
      LGX_LIB_PATH): every wave's queue lengths and stage cycles of the last launch (lgx_debug_tmq)
      and the per-workgroup phase clocks (lgx_debug_clock), under the LGX_TM_STAGE2 of the
      environment.  Writes the histogram and the cycle summary as JSON."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle_backend import make_env  # noqa: E402

FORMS = ["rows", "lane", "packed", None]


def warm(task, n):
    env = make_env(task, num_envs=n, device="cuda:0", backend="lgx")
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    for _ in range(30):
        env.step(torch.randn(n, 12, device="cuda:0", generator=g) * 0.5)
    torch.cuda.synchronize()
    return env


def forms(task, n, reps, launches):
    envs = {}
    for f in FORMS:
        if f is None:
            os.environ.pop("LGX_TM_STAGE2", None)
        else:
            os.environ["LGX_TM_STAGE2"] = f
        envs[f] = warm(task, n)
    ref = envs["lane"]
    for f, e in envs.items():
        assert torch.equal(e.root_states, ref.root_states) and torch.equal(e.dof_vel, ref.dof_vel), f
    dec = ref.cfg.control.decimation
    us = {str(f): [] for f in FORMS}
    for _ in range(reps):
        for f in FORMS:
            e = envs[f]
            state = {k: getattr(e, k).clone() for k in ("root_states", "dof_state")}
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                e.simulate(dec)
            t.record()
            t.synchronize()
            us[str(f)].append(round(1000 * s.elapsed_time(t) / launches, 2))
            for k, v in state.items():          # every repetition times the same launches
                getattr(e, k).copy_(v)
    print(json.dumps({"task": task, "num_envs": n, "launches": launches, "us_per_launch": us}), flush=True)


def hist(task, n, out):
    from legged_gym_amd.sim import lib as lgxlib
    env = warm(task, n)
    dec = env.cfg.control.decimation
    env.simulate(dec)
    torch.cuda.synchronize()
    L = lgxlib.load()
    nb = (n + 15) // 16
    pp = L.lgx_physics_lane_split(C.c_int32(n))
    tmq = np.zeros((nb, 8, 4, 4), dtype=np.uint32)
    clk = np.zeros((nb, 14), dtype=np.uint64)
    assert L.lgx_debug_tmq(tmq.ctypes.data_as(C.c_void_p), C.c_int32(nb)) == 0
    assert L.lgx_debug_clock(clk.ctypes.data_as(C.c_void_p), C.c_int32(nb)) == 0
    r = tmq[:, :pp, :dec].reshape(-1, 4).astype(np.int64)
    qn, qn2, c1, c2, form = r[:, 0] >> 16, r[:, 0] & 0xffff, r[:, 1], r[:, 2], r[:, 3]
    res = {"task": task, "num_envs": n, "pp": int(pp), "substeps": int(dec), "waves": int(nb * pp),
           "LGX_TM_STAGE2": os.environ.get("LGX_TM_STAGE2"),
           "qn_hist": {int(k): int(v) for k, v in zip(*np.unique(qn, return_counts=True))},
           "qn2_hist": {int(k): int(v) for k, v in zip(*np.unique(qn2, return_counts=True))},
           "by_qn2": {}}
    for k in np.unique(qn2):
        m = (qn2 == k) & (qn > 0)
        if m.any():
            res["by_qn2"][int(k)] = {"count": int(m.sum()), "form": int(np.bincount(form[m]).argmax()),
                                     "stage1_cycles_mean": float(c1[m].mean()), "stage2_cycles_mean": float(c2[m].mean()),
                                     "stage2_cycles_max": int(c2[m].max())}
    # per wave over the launch: the queue phase's cycles
    wave_q = (c1 + c2).reshape(nb * pp, dec).sum(1)
    res["queue_cycles_per_wave"] = {"mean": float(wave_q.mean()), "p95": float(np.percentile(wave_q, 95)),
                                    "max": int(wave_q.max())}
    # workgroups (wave 0's clocks): total = the sum of its phase clocks; the slowest 5 % against the mean
    ph = clk[:, 2:13].astype(np.int64)        # phases 0..10 (11 holds the queue lengths)
    tot = ph.sum(1)
    slow = tot >= np.percentile(tot, 95)
    wg_q = (c1 + c2).reshape(nb, pp, dec).sum(2).max(1)     # the workgroup's slowest wave in the queue phase
    res["workgroups"] = {"wave0_total_cycles_mean": float(tot.mean()), "wave0_total_cycles_max": int(tot.max()),
                         "slowest5pct_total_cycles_mean": float(tot[slow].mean()),
                         "phase_cycles_mean": [float(x) for x in ph.mean(0)],
                         "phase_cycles_slowest5pct": [float(x) for x in ph[slow].mean(0)],
                         "realtime_100MHz_ticks_mean": float((clk[:, 1] - clk[:, 0]).astype(np.int64).mean()),
                         "realtime_100MHz_ticks_max": int((clk[:, 1] - clk[:, 0]).astype(np.int64).max()),
                         "queue_cycles_slowest_wave_mean": float(wg_q.mean()),
                         "queue_cycles_slowest_wave_of_slowest5pct": float(wg_q[slow].mean())}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("LGX_TM_STAGE2", "qn_hist", "qn2_hist", "queue_cycles_per_wave")}), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    task = a[1] if len(a) > 1 else "go1_rough"
    n = int(a[2]) if len(a) > 2 else 4096
    if a and a[0] == "forms":
        forms(task, n, int(a[3]) if len(a) > 3 else 3, int(a[4]) if len(a) > 4 else 50)
    elif a and a[0] == "hist":
        hist(task, n, a[3] if len(a) > 3 else "trimesh_queue_hist.json")
    else:
        sys.exit(__doc__)
