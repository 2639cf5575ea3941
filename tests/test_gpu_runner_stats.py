"""GPU: OnPolicyRunner.learn with a log directory - the device episode statistics
(EpisodeStats / lgx_episode_stats_step, the default) against rsl_rl's torch / deque block
(LGX_DEVICE_STATS=0), and deferred logging (LGX_DEFER_LOG=1) against the synchronous run.
go1_rough, 256 envs, 3 iterations, init_at_random_ep_len (episodes end in the first rollout),
same seeds; every run is made once and shared by the tests."""
import os

import pytest
import torch

from oracle_backend import make_env

pytestmark = pytest.mark.gpu

ITERATIONS, SAVE_INTERVAL = 3, 2
SYNCING = ("cpu", "item", "tolist", "nonzero")     # torch.Tensor methods that wait for the device


class Writer:
    """Stands in for the TensorBoard SummaryWriter: keeps what log() reports."""

    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, it):
        self.scalars.append((tag, value, it))


def run(log_dir, env_vars):
    from legged_gym_amd.envs.go1.go1_config import Go1RoughCfgPPO
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    saved_env = {k: os.environ.get(k) for k in ("LGX_DEVICE_STATS", "LGX_DEFER_LOG")}
    saved_methods = {name: getattr(torch.Tensor, name) for name in SYNCING}
    rec = dict(logs=[], extras_steps=[], defer=[], syncs=0, collecting=False)
    try:
        for k in saved_env:
            os.environ.pop(k, None)
        os.environ.update(env_vars)
        env = make_env("go1_rough", num_envs=256, device="cuda:0", backend="lgx")
        cfg = class_to_dict(Go1RoughCfgPPO())
        cfg["runner"]["save_interval"] = SAVE_INTERVAL
        torch.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir, device="cuda:0")
        runner.writer = rec["writer"] = Writer()
        alg = runner.alg
        orig_act, orig_returns, orig_update, orig_log = alg.act, alg.compute_returns, alg.update, runner.log

        def counted(name):
            def method(self, *a, **kw):
                rec["syncs"] += rec["collecting"]
                return saved_methods[name](self, *a, **kw)
            return method

        def act(obs, cobs):              # the collection window: first act .. compute_returns
            rec["collecting"] = True
            return orig_act(obs, cobs)

        def compute_returns(cobs):
            rec["collecting"] = False
            return orig_returns(cobs)

        def update(defer=False):
            rec["defer"].append(defer)
            return orig_update(defer=defer)

        def log(locs, *a, **kw):
            rec["logs"].append((locs["it"], locs["mean_value_loss"], locs["mean_surrogate_loss"],
                                list(locs["rewbuffer"]), list(locs["lenbuffer"])))
            rec["extras_steps"].append({k: torch.stack([ep[k].reshape(()) for ep in locs["ep_infos"]]).double().cpu()
                                        for k in locs["ep_infos"][0]})
            return orig_log(locs, *a, **kw)

        alg.act, alg.compute_returns, alg.update, runner.log = act, compute_returns, update, log
        for name in SYNCING:
            setattr(torch.Tensor, name, counted(name))
        torch.manual_seed(7)
        runner.learn(ITERATIONS, init_at_random_ep_len=True)
        torch.cuda.synchronize()
    finally:
        for name, m in saved_methods.items():
            setattr(torch.Tensor, name, m)
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    o = alg.optimizer
    rec.update(params=[p.detach().clone() for p in alg.actor_critic.parameters()], m=o.m.clone(), v=o.v.clone(),
               lr=alg.learning_rate, pending=alg._fused._pending,
               files={f: torch.load(os.path.join(log_dir, f), weights_only=True)
                      for f in sorted(os.listdir(log_dir)) if f.endswith(".pt")})
    return rec


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    return {name: run(str(tmp_path_factory.mktemp(name)), env_vars)
            for name, env_vars in (("old", {"LGX_DEVICE_STATS": "0"}), ("new", {}), ("defer", {"LGX_DEFER_LOG": "1"}))}


def same(a, b):
    """Bitwise equality of two checkpoint values (nested dicts / lists of tensors and scalars)."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_device_statistics_match_the_deque_block(runs):
    old, new = runs["old"], runs["new"]
    assert [l[0] for l in new["logs"]] == list(range(ITERATIONS))
    assert len(new["logs"][0][3]) > 0, "episodes end in the first rollout"
    for a, b in zip(old["logs"], new["logs"]):
        assert a[3] == b[3] and a[4] == b[4], a[0]                  # reward / length lists
        assert a[:3] == b[:3], a[0]                                   # iteration, losses
    assert all(torch.equal(x, y) for x, y in zip(old["params"], new["params"]))
    assert torch.equal(old["m"], new["m"]) and torch.equal(old["v"], new["v"]) and old["lr"] == new["lr"]


def test_extras_means_in_one_readback(runs):
    """Episode/<key>: same keys, same order; the means differ from the per-key torch means by at
    most the float32 summation bound of S = 24 terms, 2 (S - 1) 2^-24 mean|v|."""
    old, new = runs["old"], runs["new"]
    tags = lambda r: [(t, it) for t, _, it in r["writer"].scalars]
    assert tags(old) == tags(new)
    assert any(t.startswith("Episode/") for t, _ in tags(new))
    for (tag, a, it), (_, b, _) in zip(old["writer"].scalars, new["writer"].scalars):
        if not tag.startswith("Episode/"):
            continue
        v = new["extras_steps"][it][tag[len("Episode/"):]]
        S = v.numel()
        assert S == 24
        bound = 2 * (S - 1) * 2.0 ** -24 * float(v.abs().mean())
        print(f"{tag} it {it}: old {a!r} new {b!r} |diff| {abs(a - b):.3e} bound {bound:.3e}")
        assert abs(a - b) <= bound, (tag, it, a, b, bound)
        assert abs(b - float(v.mean())) <= bound, (tag, it)


def test_no_host_sync_during_collection(runs):
    """No Tensor.cpu / .item / .tolist / .nonzero between an iteration's first act and its
    compute_returns with the device statistics; the deque block makes two gathers per step."""
    assert runs["old"]["syncs"] > 0
    assert runs["new"]["syncs"] == 0
    assert runs["defer"]["syncs"] == 0


def test_deferred_logging_matches_synchronous(runs):
    new, defer = runs["new"], runs["defer"]
    assert new["defer"] == [False] * ITERATIONS
    assert defer["defer"] == [it % SAVE_INTERVAL != 0 for it in range(ITERATIONS)] == [False, True, False]
    assert defer["logs"] == new["logs"]           # (it, value loss, surrogate loss, rewards, lengths)
    mean = lambda r: [(sum(l[3]) / len(l[3]), sum(l[4]) / len(l[4])) for l in r["logs"]]
    assert mean(defer) == mean(new)
    reported = lambda r: [s for s in r["writer"].scalars if not s[0].startswith("Perf/")]   # (all but the timings)
    assert reported(defer) == reported(new)
    assert list(defer["files"]) == list(new["files"]) == ["model_0.pt", "model_2.pt", "model_3.pt"]
    for f in new["files"]:
        assert same(defer["files"][f], new["files"][f]), f
    assert defer["pending"] is None and new["pending"] is None
    assert all(torch.equal(x, y) for x, y in zip(defer["params"], new["params"]))
