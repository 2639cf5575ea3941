"""GPU: left-right symmetry augmentation (rsl_rl 2.x symmetry_cfg.use_data_augmentation; DESIGN.md
§4.3e): lgx_ppo_symmetry_augment against numpy (bitwise: a copy and a sign flip), the physical check
of the tables' signs on the lgx physics, the fused update over real rows + mirrors against autograd,
and what the feature is for: an equivariant policy stays equivariant.

Tolerances: minibatch gradient |d| <= 1e-5 + 2e-3 |g| and the full-update criteria of
tests/test_gpu_ppo.py; observations 2e-3 + 2e-3 |x| (velocity columns) / 1e-4 (tests/test_gpu_parity.py).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import symmetry_ref as sr
from legged_gym_amd.rl.actor_critic import ActorCritic
from legged_gym_amd.rl.ppo import PPO
from legged_gym_amd.sim import abi
from legged_gym_amd.utils.task_registry import task_registry
from oracle_backend import make_env
from test_gpu_parity import sync
from test_gpu_ppo import _CallCounter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SYM_ON = {"use_data_augmentation": True}
T, N, ACT = 6, 64, 12
B = T * N
SCALARS = ("actions_log_prob", "advantages", "values", "returns")


def cfg_of(task):
    return type(task_registry.get_cfgs(task)[0])()


@pytest.fixture(scope="module")
def tables(gpu):
    """Go1 tables on the device: obs 235 (go1_rough) / 475 (go1_rough_hist), critic 253 (go1_rough_asym)."""
    asym = sr.as_tensors(sr.cfg_tables(cfg_of("go1_rough_asym")), DEV)
    hist = sr.as_tensors(sr.cfg_tables(cfg_of("go1_rough_hist")), DEV)
    return {235: asym["obs"], 253: asym["critic_obs"], 475: hist["obs"], "actions": asym["actions"]}


def pick(tables, obs, cobs):
    return {"obs": tables[obs], "critic_obs": tables[cobs] if cobs else None, "actions": tables["actions"]}


# ---------------------------------------------------------------- the kernel against numpy
def launch(lib, arrays, tab, rows, src_row, dst_row):
    a = abi.LgxSymmetryArgs()
    a.rows, a.src_row, a.dst_row = rows, src_row, dst_row
    a.num_obs, a.num_actions = arrays["observations"].shape[1], ACT
    for name, x in arrays.items():
        setattr(a, name, x.data_ptr())
    a.obs_perm, a.obs_sign = tab["obs"][0].data_ptr(), tab["obs"][1].data_ptr()
    a.act_perm, a.act_sign = tab["actions"][0].data_ptr(), tab["actions"][1].data_ptr()
    if "privileged_observations" in arrays:
        a.num_cobs = arrays["privileged_observations"].shape[1]
        a.cobs_perm, a.cobs_sign = tab["critic_obs"][0].data_ptr(), tab["critic_obs"][1].data_ptr()
    rc = lib.lgx_ppo_symmetry_augment(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.lgx_last_error()
    torch.cuda.synchronize()


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.mark.parametrize("rows", [37, 4])                      # 37: not a multiple of the 4 rows per workgroup
# 475: more than one 256-column pass, and no privileged array
@pytest.mark.parametrize("obs,cobs", [(235, 253), (475, None)])
def test_augment_kernel_matches_numpy_bitwise(gpu, tables, rows, obs, cobs):
    from legged_gym_amd.sim import lib as lgxlib
    lib = lgxlib.load()
    tab = pick(tables, obs, cobs)
    CANARY = 3
    g = torch.Generator(device=DEV).manual_seed(rows + obs)
    widths = {"observations": obs, "actions": ACT, "mu": ACT, "sigma": ACT, **{k: 1 for k in SCALARS}}
    if cobs:
        widths["privileged_observations"] = cobs
    arrays = {k: torch.randn(2 * rows + CANARY, w, device=DEV, generator=g) for k, w in widths.items()}
    for x in arrays.values():
        x[rows:2 * rows] = 7.0          # the mirror half starts as junk
    before = {k: x.clone() for k, x in arrays.items()}
    launch(lib, arrays, tab, rows, 0, rows)
    host_tab = {k: None if v is None else (v[0].cpu().numpy(), v[1].cpu().numpy()) for k, v in tab.items()}
    want = sr.augment_numpy({k: x.cpu().numpy() for k, x in before.items()}, host_tab, rows)
    for k, x in arrays.items():
        assert np.array_equal(bits(x[:rows]), bits(before[k][:rows])), k                   # real rows unchanged
        assert np.array_equal(bits(x[rows:2 * rows]), want[k].astype(np.float32).view(np.int32)), k
        assert np.array_equal(bits(x[2 * rows:]), bits(before[k][2 * rows:])), k           # canary untouched
    assert not torch.equal(arrays["observations"][rows:2 * rows], arrays["observations"][:rows])
    # the mirror of the mirror half is the real half
    for x in arrays.values():
        x[:rows] = 9.0
    launch(lib, arrays, tab, rows, rows, 0)
    for k, x in arrays.items():
        assert np.array_equal(bits(x[:rows]), bits(before[k][:rows])), k
        assert np.array_equal(bits(x[2 * rows:]), bits(before[k][2 * rows:])), k


# ---------------------------------------------------------------- physical check on the lgx backend
def test_lgx_dynamics_commute_with_the_mirror(gpu):
    """tests/test_symmetry.py::test_oracle_dynamics_commute_with_the_mirror on the lgx backend (the
    same construction and bounds, the same mirror-symmetric Go1 model), and lgx against the oracle."""
    ora = sr.mirrored_envs()
    dev = sr.mirrored_envs(device=DEV, backend="lgx")
    tab = ora[0].symmetry_tables()
    a = sr.smooth_state(ora[0], torch.Generator().manual_seed(5))
    sr.reflect_state(ora[0], ora[1], tab)
    sr.assert_pd_unsaturated(ora[0], a)
    acts = (a, sr.mirror(a, tab["actions"]))
    for o, d, act in zip(ora, dev, acts):
        sync(o, d)
        o.common_step_counter = d.common_step_counter = 3
        o.step(act)
        d.step(act.to(DEV))
    torch.cuda.synchronize()
    for env in (*ora, *dev):
        sr.assert_smooth(env)
    dtab = dev[0].symmetry_tables()
    assert dtab["obs"][0].is_cuda and torch.equal(dtab["obs"][0].cpu(), tab["obs"][0])
    sr.assert_obs_close(dev[1].obs_buf, sr.mirror(dev[0].obs_buf, dtab["obs"]), "lgx: obs(mirror state) vs mirror(obs)")
    for k in range(2):
        sr.assert_obs_close(dev[k].obs_buf, ora[k].obs_buf, f"lgx vs oracle, env {'AB'[k]}")


# ---------------------------------------------------------------- fused update over rows + mirrors
def make_sym_pair(tab, schedule="adaptive", cobs=None, epochs=2, symmetry=SYM_ON, seed=3, prepare=None, obs=235):
    """tests/test_gpu_ppo.py make_pair with symmetry augmentation: reference (autograd, torch
    mirroring) and fused PPO on identical T x N storage, 4 minibatches."""
    torch.manual_seed(0)
    ac = ActorCritic(obs, cobs or obs, ACT, [512, 256, 128], [512, 256, 128])
    if prepare:
        prepare(ac)
    ac2 = copy.deepcopy(ac)
    kw = dict(num_learning_epochs=epochs, num_mini_batches=4, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0,
              entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0, schedule=schedule, desired_kl=0.01,
              device=DEV, symmetry=symmetry)
    ref = PPO(ac, use_fused_update=False, **kw)
    fus = PPO(ac2, use_fused_update=True, **kw)
    assert fus._fused is not None and ref._fused is None
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    data = dict(observations=r(T, N, obs), actions=r(T, N, ACT), rewards=r(T, N, 1), values=r(T, N, 1),
                dones=(torch.rand(T, N, 1, device=DEV, generator=g) < 0.1).byte(),
                actions_log_prob=r(T, N, 1) * 0.3 - 17, mu=r(T, N, ACT) * 0.1,
                sigma=torch.rand(T, N, ACT, device=DEV, generator=g) * 0.5 + 0.75)
    if cobs:
        data["privileged_observations"] = r(T, N, cobs)
    last = r(N, 1)
    for p in (ref, fus):
        if symmetry:
            p.init_symmetry(tab)
        p.init_storage(N, T, [obs], [cobs], [ACT])
        for name, x in data.items():
            getattr(p.storage, name).copy_(x)
        p.storage.step = T
        p.storage.compute_returns(last, 0.99, 0.95)
    return ref, fus


def autograd_grads_mirrored(ref, idx, tab):
    """Autograd gradient of the PPO loss on rows idx and their torch-mirrored images, concatenated."""
    st, ac = ref.storage, ref.actor_critic
    both = lambda x, t=None: torch.cat((x, sr.mirror(x, t) if t is not None else x))
    flat = lambda name: getattr(st, name).reshape(B, -1)[idx]
    obs = both(flat("observations"), tab["obs"])
    cobs = both(flat("privileged_observations"), tab["critic_obs"]) if st.privileged_observations is not None else obs
    ac.act(obs)
    logp = ac.get_actions_log_prob(both(flat("actions"), tab["actions"]))
    value = ac.evaluate(cobs)
    ratio = torch.exp(logp - both(flat("actions_log_prob")).squeeze(1))
    adv = both(flat("advantages")).squeeze(1)
    s = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    tv, ret = both(flat("values")), both(flat("returns"))
    vc = tv + (value - tv).clamp(-0.2, 0.2)
    vl = torch.max((value - ret).pow(2), (vc - ret).pow(2)).mean()
    loss = s + vl - 0.01 * ac.entropy.mean()
    for p in ac.parameters():
        p.grad = None
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in ac.named_parameters()}


@pytest.mark.parametrize("cobs", [None, 253])
@pytest.mark.parametrize("rows", [384, 37])
def test_fused_gradient_over_rows_and_mirrors(gpu, tables, rows, cobs):
    tab = pick(tables, 235, cobs)
    ref, fus = make_sym_pair(tab, cobs=cobs)
    st = fus.storage
    assert st.full("observations").shape == (2 * T, N, 235) and st.observations.shape == (T, N, 235)
    # advantage statistics are the real rows' alone
    adv = st.returns - st.values
    assert torch.allclose(st.advantages, (adv - adv.mean()) / (adv.std() + 1e-8), atol=1e-5)
    idx = torch.randperm(B, device=DEV)[:rows]
    gref = autograd_grads_mirrored(ref, idx, tab)
    fus._fused.augment()
    fus._fused.gradients(torch.cat((idx, idx + B)))
    for n, p in fus.actor_critic.named_parameters():
        a, b = p.grad, gref[n]
        assert ((a - b).abs() <= 1e-5 + 2e-3 * b.abs()).all(), (n, (a - b).abs().max().item(), b.abs().max().item())


def test_fused_update_matches_autograd_update_with_symmetry(gpu, tables):
    """The criteria of test_gpu_ppo.py::test_fused_update_matches_autograd_update, 2 epochs x 4
    minibatches of 96 rows + 96 mirrors, adaptive schedule (KL over all 192 rows on both paths)."""
    tab = pick(tables, 235, None)
    ref, fus = make_sym_pair(tab)
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    fus._fused.lib = spy = _CallCounter(fus._fused.lib)
    vl_f, sl_f = fus.update()
    assert spy.calls.get("lgx_ppo_symmetry_augment", 0) == 1            # once per update
    assert spy.calls.get("lgx_adam_clip_mirror_sq", 0) == 8             # the number of minibatches is unchanged
    assert fus.learning_rate == ref.learning_rate
    assert abs(vl_f - vl_r) <= 1e-4 * abs(vl_r) + 1e-6 and abs(sl_f - sl_r) <= 1e-4 * abs(sl_r) + 1e-6
    big = total = 0
    for a, b in zip(fus.actor_critic.parameters(), ref.actor_critic.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    assert big <= 1e-3 * total, (big, total)
    # both paths wrote the same mirror half
    for name in ("observations", "actions", "mu", "sigma", "advantages"):
        assert torch.equal(fus.storage.full(name), ref.storage.full(name)), name


# ---------------------------------------------------------------- equivariance is preserved
def make_equivariant(tab):
    """prepare(actor_critic): the actor made exactly mirror-equivariant, actor(mirror(o)) ==
    mirror(actor(o)) in exact arithmetic: hidden units in swapped pairs (2i <-> 2i + 1), layer 1
    symmetrised with the observation table, the head with the action table, W <- (W + Q W P) / 2
    (a + b is commutative in floating point: paired entries are bitwise equal up to the sign)."""
    cpu = {k: None if v is None else (v[0].cpu(), v[1].cpu()) for k, v in tab.items()}

    def swap(n):
        return torch.arange(n).view(-1, 2).flip(1).reshape(-1)

    def prepare(ac):
        lin = [m for m in ac.actor if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for k, l in enumerate(lin):
                W, b = l.weight, l.bias
                Wp = sr.mirror(W, cpu["obs"]) if k == 0 else W[:, swap(W.shape[1])]         # W P (columns)
                if k == len(lin) - 1:                                                    # Q (rows): the action table
                    p, s = cpu["actions"][0].long(), cpu["actions"][1]
                    W.copy_((W + s[:, None] * Wp[p]) / 2)
                    b.copy_((b + s * b[p]) / 2)
                else:
                    q = swap(W.shape[0])
                    W.copy_((W + Wp[q]) / 2)
                    b.copy_((b + b[q]) / 2)
    return prepare


def equivariance_defect(ac, tab, o):
    """max |actor(mirror(o)) - mirror(actor(o))| / (1 + |.|), evaluated in float64 (the forward's own
    rounding out of the way: what is left is the weights' asymmetry)."""
    actor = copy.deepcopy(ac.actor).double()
    o = o.double()
    to64 = lambda t: (t[0], t[1].double())
    with torch.no_grad():
        lhs = actor(sr.mirror(o, to64(tab["obs"])))
        rhs = sr.mirror(actor(o), to64(tab["actions"]))
    return ((lhs - rhs).abs() / (1 + rhs.abs())).max().item()


def test_augmentation_keeps_an_equivariant_actor_equivariant(gpu, tables):
    """An exactly equivariant actor, one fused update (1 epoch x 4 minibatches, fixed lr 1e-3).  With
    augmentation every minibatch is closed under the mirror, so the gradient - and Adam's elementwise
    step - keeps the weights' symmetry up to the gradient's rounding: paired weights receive steps
    that differ by at most the relative gradient bound, 2e-3, of a step; Adam's step is at most lr per
    coordinate, so after n steps the defect is bounded by 2e-3 x n x lr = 8e-6 (relative to 1 + |a|).
    Without augmentation the steps of paired weights are unrelated (order lr each): the defect must
    exceed 10 x that bound - which is what shows the feature does something."""
    tab = pick(tables, 235, None)
    prepare = make_equivariant(tab)
    lr, steps = 1e-3, 1 * 4
    bound = 2e-3 * steps * lr
    o = torch.randn(64, 235, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    _, sym = make_sym_pair(tab, schedule="fixed", epochs=1, prepare=prepare)
    _, plain = make_sym_pair(tab, schedule="fixed", epochs=1, prepare=prepare, symmetry=None)
    start = equivariance_defect(sym.actor_critic, tab, o)
    assert start <= 1e-12, start
    before = [p.detach().clone() for p in sym.actor_critic.actor.parameters()]
    for p in (sym, plain):
        torch.manual_seed(11)
        p.update()
    assert any(not torch.equal(a, b) for a, b in zip(before, sym.actor_critic.actor.parameters()))
    d_sym = equivariance_defect(sym.actor_critic, tab, o)
    d_plain = equivariance_defect(plain.actor_critic, tab, o)
    print(f"equivariance defect: start {start:.2e}, after an augmented update {d_sym:.2e}, after a plain update "
          f"{d_plain:.2e}; bound {bound:.2e}")
    assert d_sym <= bound, (d_sym, bound)
    assert d_plain > 10 * bound, (d_plain, bound)


# ---------------------------------------------------------------- symmetry off, end to end
def test_symmetry_off_changes_nothing(gpu, tables):
    _, fus = make_sym_pair(pick(tables, 235, None), symmetry=None)
    st = fus.storage
    assert st.symmetry is None and st.observations.shape == (T, N, 235) and st.full("observations") is st.observations
    for name in ("actions", "mu", "sigma"):
        assert getattr(st, name).shape == (T, N, ACT) and getattr(st, name).untyped_storage().nbytes() == B * ACT * 4
    for name in SCALARS:
        assert getattr(st, name).shape == (T, N, 1) and getattr(st, name).untyped_storage().nbytes() == B * 4
    assert st.observations.untyped_storage().nbytes() == B * 235 * 4
    fus._fused.lib = spy = _CallCounter(fus._fused.lib)
    torch.manual_seed(11)
    fus.update()
    assert spy.calls.get("lgx_ppo_symmetry_augment", 0) == 0 and spy.calls.get("lgx_adam_clip_mirror_sq", 0) == 8
    with pytest.raises(ValueError, match="no symmetry tables"):
        fus._fused.augment()


def test_go1_rough_sym_end_to_end(gpu, tmp_path):
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    env = make_env("go1_rough_sym", num_envs=64, device=DEV, backend="lgx")
    cfg = class_to_dict(task_registry.get_cfgs("go1_rough_sym")[1])
    assert cfg["algorithm"]["symmetry"] == SYM_ON
    torch.manual_seed(0)
    runner = OnPolicyRunner(env, cfg, str(tmp_path), device=DEV)
    st = runner.alg.storage
    assert runner.alg._fused is not None and st.symmetry is not None and st.full("observations").shape[0] == 2 * 24
    runner.alg._fused.lib = spy = _CallCounter(runner.alg._fused.lib)
    runner.learn(2, init_at_random_ep_len=True)
    assert spy.calls.get("lgx_ppo_symmetry_augment", 0) == 2
    stats = runner.last_iteration_stats
    assert np.isfinite([stats["value_loss"], stats["surrogate_loss"], stats["learning_rate"]]).all(), stats
    Bn = 24 * 64
    obs = st.full("observations").view(2 * Bn, -1)
    assert torch.equal(obs[Bn:], sr.mirror(obs[:Bn], st.symmetry["obs"]))
    path = tmp_path / "model_2.pt"
    assert path.exists()
    other = OnPolicyRunner(env, cfg, None, device=DEV)
    other.load(str(path))
    for a, b in zip(runner.alg.actor_critic.parameters(), other.alg.actor_critic.parameters()):
        assert torch.equal(a, b)
    assert other.current_learning_iteration == 2
