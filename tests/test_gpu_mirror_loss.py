"""GPU: the symmetry mirror loss on the fused update (rsl_rl 2.x symmetry_cfg.use_mirror_loss; DESIGN.md
§4.3f): lgx_ppo_loss_bwd_mirror on its own against the float64 statement of tests/mirror_loss_ref.py,
the fused minibatch gradient and the whole update against the unfused path, what the term is for (the
equivariance defect shrinks), off meaning off, and go1_rough_mirror end to end.

Tolerances are those of tests/test_gpu_symmetry.py: gradient |d| <= 1e-5 + 2e-3 |g|, losses 1e-4, and the
full-update criteria of tests/test_gpu_ppo.py (at most 1e-3 of the parameters off by more than 1e-5).
"""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mirror_loss_ref as ml
import symmetry_ref as sr
from legged_gym_amd.sim import abi
from legged_gym_amd.utils.task_registry import task_registry
from oracle_backend import make_env
from test_gpu_ppo import _CallCounter
from test_gpu_symmetry import ACT, B, DEV, N, SYM_ON, T, bits, make_sym_pair, pick, tables  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

COEFF = 0.5
MIRROR = {"use_mirror_loss": True, "mirror_loss_coeff": COEFF}                 # (B): the mirror loss alone
BOTH = {"use_data_augmentation": True, **MIRROR}                               # (A): on top of the augmentation
COMBOS = pytest.mark.parametrize("symmetry", [BOTH, MIRROR], ids=["augment+mirror", "mirror"])
EINVAL = -1


def close(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    assert (err <= 1e-5 + 2e-3 * b.abs()).all(), (what, err.max().item(), b.abs().max().item())


def loss_close(a, b, what):
    assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (what, a, b)


# ---------------------------------------------------------------- the launch alone
H, CANARY = 128, 64


class Launch:
    """Inputs and output buffers of one lgx_ppo_loss_bwd_mirror call over M real rows + M mirrors, with a
    canary block behind head_in and behind every partial buffer."""

    def __init__(self, lib, tab, M, ppo_rows, seed=0):
        self.lib, self.M, self.R, self.ppo_rows = lib, M, 2 * M, ppo_rows
        R = self.R
        g = torch.Generator(device=DEV).manual_seed(seed + M)
        r = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.A3 = torch.nn.functional.elu(r(2, R, H))                     # post-ELU activations
        self.W4a, self.b4a, self.W4c, self.b4c = r(ACT, H) * 0.1, r(ACT) * 0.1, r(1, H) * 0.1, r(1) * 0.1
        self.std = torch.rand(ACT, device=DEV, generator=g) * 0.5 + 0.75
        self.idx = torch.randperm(R, device=DEV, generator=g)
        self.store = dict(actions=r(R, ACT), old_logp=r(R) * 0.3 - 17, old_mu=r(R, ACT) * 0.1,
                          old_sigma=torch.rand(R, ACT, device=DEV, generator=g) * 0.5 + 0.75, advantages=r(R),
                          target_values=r(R), returns=r(R))
        self.batch = {k: v[self.idx] for k, v in self.store.items()}       # minibatch row order, for the reference
        if ppo_rows == M:      # the mirror rows' storage is not read: poison it
            for v in self.store.values():
                v[self.idx[M:]] = float("nan")
        self.perm, self.sign = tab["actions"]
        lay = (C.c_int64 * 3)()
        assert lib.lgx_ppo_loss_bwd_layout(R, ACT, H, lay) == 0
        self.wgs = int(lib.lgx_ppo_mirror_partials_floats(R))
        assert self.wgs == -(-M // 16) == int(lay[0]) // (2 * ACT + 4)
        self.sizes = dict(head_in=2 * R * H, partials=int(lay[0]), head_parts=int(lay[1]), sym_parts=self.wgs)
        self.reset()

    def reset(self):
        self.buf = {k: torch.full((n + CANARY,), 777.0, device=DEV) for k, n in self.sizes.items()}
        self.buf["head_in"][:self.sizes["head_in"]].copy_(self.A3.reshape(-1))
        self.out = {k: torch.zeros(n, device=DEV) for k, n in dict(g_std=ACT, g_b4a=ACT, g_b4c=1, stats=3, dmu=self.R * ACT,
                                                                   dv=self.R, lsym=1).items()}

    def args(self, **over):
        a = abi.LgxPpoLossArgs()
        a.rows, a.num_actions, a.use_clipped_value_loss = self.R, ACT, 1
        a.clip_param, a.value_loss_coef, a.entropy_coef = 0.2, 1.0, 0.01
        a.idx = self.idx.data_ptr()
        a.b4a, a.b4c, a.std = self.b4a.data_ptr(), self.b4c.data_ptr(), self.std.data_ptr()
        for k, v in self.store.items():
            setattr(a, k, v.data_ptr())
        a.d_mu, a.d_v, a.partials = self.out["dmu"].data_ptr(), self.out["dv"].data_ptr(), self.buf["partials"].data_ptr()
        a.g_std, a.g_b4a, a.g_b4c = (self.out[k].data_ptr() for k in ("g_std", "g_b4a", "g_b4c"))
        a.stats, a.lr, a.desired_kl = self.out["stats"].data_ptr(), None, 0.0
        a.head_in, a.hidden = self.buf["head_in"].data_ptr(), H
        a.W4a, a.W4c = self.W4a.data_ptr(), self.W4c.data_ptr()
        a.defer_finalize = 0                                              # the finalize launch follows at once
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, args=None, **over):
        kw = dict(perm=self.perm.data_ptr(), sign=self.sign.data_ptr(), coeff=COEFF, ppo_rows=self.ppo_rows,
                  sym=self.buf["sym_parts"].data_ptr())
        kw.update(over)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.lgx_ppo_loss_bwd_mirror(C.byref(args or self.args()), C.c_void_p(kw["perm"]), C.c_void_p(kw["sign"]),
                                              kw["coeff"], kw["ppo_rows"], C.c_void_p(kw["sym"]),
                                              C.c_void_p(self.buf["head_parts"].data_ptr()), stream)
        torch.cuda.synchronize()
        return rc

    def results(self):
        """Everything the launch (+ its finalize, + the symmetry reduction) wrote, as host tensors."""
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.lgx_ppo_mirror_loss_reduce(C.c_void_p(self.buf["sym_parts"].data_ptr()), self.wgs,
                                                 1.0 / (self.M * ACT), C.c_void_p(self.out["lsym"].data_ptr()), stream)
        assert rc == 0, self.lib.lgx_last_error()
        torch.cuda.synchronize()
        n = self.sizes
        hp = self.buf["head_parts"][:n["head_parts"]].view(self.wgs, (ACT + 1) * H + 2 * H).double().sum(0)
        res = dict(dZ3=self.buf["head_in"][:n["head_in"]].view(2, self.R, H), dW4a=hp[:ACT * H].view(ACT, H),
                   dW4c=hp[ACT * H:(ACT + 1) * H].view(1, H), db3=hp[(ACT + 1) * H:].view(2, H),
                   **{k: self.out[k] for k in ("g_std", "g_b4a", "g_b4c", "stats", "lsym")})
        return {k: v.detach().cpu().clone() for k, v in res.items()}

    def canaries_intact(self):
        return all((self.buf[k][n:] == 777.0).all().item() for k, n in self.sizes.items())

    def raw(self):
        return {k: bits(v) for k, v in {**self.buf, **{k: self.out[k] for k in ("g_std", "g_b4a", "g_b4c", "stats")}}.items()}


@pytest.mark.parametrize("both", [True, False], ids=["ppo_rows=2M", "ppo_rows=M"])
@pytest.mark.parametrize("M", [5, 37, 48])      # one partial workgroup; two full pair-chunks + a 5-pair tail; exact
def test_launch_matches_the_float64_statement(gpu, tables, M, both):
    from legged_gym_amd.sim import lib as lgxlib
    lib = lgxlib.load()
    L = Launch(lib, pick(tables, 235, None), M, 2 * M if both else M)
    assert L.call() == 0, lib.lgx_last_error()
    got, first = L.results(), L.raw()
    assert L.canaries_intact()
    want = ml.head_reference(L.A3, L.W4a, L.b4a, L.W4c, L.b4c, L.std, L.batch, L.ppo_rows, COEFF, L.perm, L.sign)
    for k in ("dZ3", "dW4a", "dW4c", "db3", "g_std", "g_b4a", "g_b4c"):
        assert torch.isfinite(got[k]).all(), k
        close(got[k], want[k], k)
    print(f"M {M} ppo_rows {L.ppo_rows}: KL {got['stats'][0]:.6f} / {want['kl']:.6f}, surrogate {got['stats'][1]:.6f} / "
          f"{want['surrogate']:.6f}, value {got['stats'][2]:.6f} / {want['value_loss']:.6f}, L_sym {got['lsym'][0]:.6f} / "
          f"{want['symmetry']:.6f}")
    for i, k in enumerate(("kl", "surrogate", "value_loss")):
        loss_close(got["stats"][i].item(), want[k], k)
    loss_close(got["lsym"][0].item(), want["symmetry"], "L_sym")
    if not both:      # the mirror rows carry the mirror term only: their critic rows get no gradient
        assert not got["dZ3"][1, M:].any()
    # the same inputs again: the same bits everywhere
    L.reset()
    assert L.call() == 0
    L.results()
    second = L.raw()
    for k in first:
        assert np.array_equal(first[k], second[k]), k


def test_launch_refuses_bad_arguments(gpu, tables):
    from legged_gym_amd.sim import lib as lgxlib
    lib = lgxlib.load()
    L = Launch(lib, pick(tables, 235, None), 5, 5)
    before = L.raw()
    odd = L.args(rows=9)
    cases = [("odd rows", dict(args=odd, ppo_rows=9), "even"),
             ("ppo_rows", dict(ppo_rows=7), "ppo_rows"), ("ppo_rows 0", dict(ppo_rows=0), "ppo_rows"),
             ("null perm", dict(perm=None), "null"), ("null sign", dict(sign=None), "null"),
             ("null partials", dict(sym=None), "null"),
             ("coeff 0", dict(coeff=0.0), "coeff"), ("coeff < 0", dict(coeff=-1.0), "coeff"),
             ("coeff inf", dict(coeff=math.inf), "coeff"), ("coeff nan", dict(coeff=math.nan), "coeff"),
             ("no head_in", dict(args=L.args(head_in=None)), "head_in")]
    for what, kw, msg in cases:
        assert L.call(**kw) == EINVAL, what
        assert msg in lib.lgx_last_error().decode(), (what, lib.lgx_last_error())
        after = L.raw()
        for k in before:                                                  # nothing was launched
            assert np.array_equal(before[k], after[k]), (what, k)
    assert lib.lgx_ppo_mirror_loss_reduce(None, 1, 1.0, None, None) == EINVAL


# ---------------------------------------------------------------- the fused minibatch against autograd
def unfused_batch(ref, idx):
    """The unfused path's minibatch over storage rows idx and their mirrors (mini_batch_generator's tuple)."""
    st = ref.storage
    st.augment()
    rows = torch.cat((idx, idx + B))
    flat = lambda name: st.full(name).flatten(0, 1)[rows]
    obs = flat("observations")
    cobs = flat("privileged_observations") if st.privileged_observations is not None else obs
    return (obs, cobs, flat("actions"), flat("values"), flat("advantages"), flat("returns"), flat("actions_log_prob"),
            flat("mu"), flat("sigma"), (None, None), None)


def autograd_grads(ref, idx):
    loss, _, _, lsym, _ = ref.minibatch_loss(unfused_batch(ref, idx))
    for p in ref.actor_critic.parameters():
        p.grad = None
    loss.backward()
    return {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
            for n, p in ref.actor_critic.named_parameters()}, lsym.item()


def fused_grads(fus, idx):
    fus._fused.augment()
    fus._fused.gradients(torch.cat((idx, idx + B)))
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in fus.actor_critic.named_parameters()}, fus._fused.sym_stat.item()


def ppo_terms_off(*ppos):
    """Advantages 0, no value loss, no entropy bonus: the whole loss is coeff x L_sym."""
    for p in ppos:
        p.value_loss_coef = p.entropy_coef = 0.0
        p.storage.advantages.zero_()


@pytest.mark.parametrize("cobs", [None, 253])
@pytest.mark.parametrize("rows", [384, 37])
def test_mirror_term_in_isolation(gpu, tables, rows, cobs):
    ref, fus = make_sym_pair(pick(tables, 235, cobs), cobs=cobs, symmetry=MIRROR)
    ppo_terms_off(ref, fus)
    idx = torch.randperm(B, device=DEV)[:rows]
    gref, lref = autograd_grads(ref, idx)
    got, lsym = fused_grads(fus, idx)
    loss_close(lsym, lref, "L_sym")
    assert lref > 1e-3
    for n, g in got.items():
        if n.startswith("critic") or n == "std":
            assert not g.any() and not gref[n].any(), n                  # exactly 0: the term reaches neither
        else:
            assert gref[n].abs().max() > 0, n
            close(g, gref[n], n)


@COMBOS
@pytest.mark.parametrize("cobs", [None, 253])
@pytest.mark.parametrize("rows", [384, 37])
def test_full_gradient(gpu, tables, rows, cobs, symmetry):
    ref, fus = make_sym_pair(pick(tables, 235, cobs), cobs=cobs, symmetry=symmetry)
    idx = torch.randperm(B, device=DEV)[:rows]
    gref, lref = autograd_grads(ref, idx)
    got, lsym = fused_grads(fus, idx)
    loss_close(lsym, lref, "L_sym")
    for n, g in got.items():
        close(g, gref[n], n)


# ---------------------------------------------------------------- the whole update
@COMBOS
def test_fused_update_matches_the_unfused_update(gpu, tables, symmetry):
    """2 epochs x 4 minibatches of 96 rows + 96 mirrors, adaptive schedule."""
    ref, fus = make_sym_pair(pick(tables, 235, None), symmetry=symmetry)
    torch.manual_seed(11)
    vl_r, sl_r = ref.update()
    torch.manual_seed(11)
    fus._fused.lib = spy = _CallCounter(fus._fused.lib)
    vl_f, sl_f = fus.update()
    assert spy.calls.get("lgx_ppo_loss_bwd_mirror", 0) == 8 and spy.calls.get("lgx_ppo_loss_bwd", 0) == 0
    assert spy.calls.get("lgx_ppo_symmetry_augment", 0) == 1 and spy.calls.get("lgx_ppo_mirror_loss_reduce", 0) == 1
    assert spy.calls.get("lgx_adam_clip_mirror_sq", 0) == 8
    print(f"lr {fus.learning_rate} / {ref.learning_rate}; value {vl_f:.6f} / {vl_r:.6f}; surrogate {sl_f:.6f} / {sl_r:.6f}; "
          f"symmetry {fus.symmetry_loss:.6f} / {ref.symmetry_loss:.6f}")
    assert fus.learning_rate == ref.learning_rate                          # the same learning-rate sequence
    loss_close(vl_f, vl_r, "value")
    loss_close(sl_f, sl_r, "surrogate")
    loss_close(fus.symmetry_loss, ref.symmetry_loss, "symmetry")
    assert ref.symmetry_loss > 0
    big = total = 0
    for a, b in zip(fus.actor_critic.parameters(), ref.actor_critic.parameters()):
        d = (a - b).abs()
        big += (d > 1e-5).sum().item()
        total += d.numel()
    assert big <= 1e-3 * total, (big, total)
    # a deferred update resolves to the same three losses
    _, fus2 = make_sym_pair(pick(tables, 235, None), symmetry=symmetry)
    torch.manual_seed(11)
    assert fus2.update(defer=True) is None and fus2.symmetry_loss is None
    vl_d, sl_d = fus2.resolve()
    for got, want, what in ((vl_d, vl_f, "value"), (sl_d, sl_f, "surrogate"), (fus2.symmetry_loss, fus.symmetry_loss, "symmetry")):
        loss_close(got, want, "deferred " + what)


def defect64(ppo, tab, o):
    """L_sym of the actor on the fixed observations o, evaluated in float64."""
    actor = copy.deepcopy(ppo.actor_critic.actor).double()
    to64 = lambda t: (t[0], t[1].double())
    with torch.no_grad():
        mu = actor(torch.cat((o.double(), sr.mirror(o.double(), to64(tab["obs"])))))
        return ml.symmetry_loss(mu, *tab["actions"]).item()


def test_one_update_shrinks_the_equivariance_defect(gpu, tables):
    """PPO terms off, a random actor, one update (1 epoch x 4 minibatches, fixed lr): every step descends
    coeff x L_sym alone, so L_sym on a fixed batch must come out strictly smaller, on both paths alike."""
    tab = pick(tables, 235, None)
    ref, fus = make_sym_pair(tab, schedule="fixed", epochs=1, symmetry=MIRROR)
    ppo_terms_off(ref, fus)
    o = torch.randn(64, 235, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    before = defect64(fus, tab, o)
    assert before == defect64(ref, tab, o) and before > 1e-3
    after = []
    for p in (ref, fus):
        torch.manual_seed(11)
        p.update()
        after.append(defect64(p, tab, o))
    print(f"L_sym on the fixed batch: {before:.6f} -> unfused {after[0]:.6f}, fused {after[1]:.6f}")
    assert after[0] < before and after[1] < before
    loss_close(after[1], after[0], "L_sym after")


# ---------------------------------------------------------------- off is off, and refusals of the plan
def test_mirror_loss_off_changes_nothing(gpu, tables):
    tab = pick(tables, 235, None)
    params = []
    for symmetry in ({"use_data_augmentation": True, "use_mirror_loss": False}, SYM_ON):
        _, fus = make_sym_pair(tab, symmetry=symmetry)
        fus._fused.lib = spy = _CallCounter(fus._fused.lib)
        torch.manual_seed(11)
        fus.update()
        assert spy.calls.get("lgx_ppo_loss_bwd", 0) == 8 and spy.calls.get("lgx_ppo_loss_bwd_mirror", 0) == 0
        assert spy.calls.get("lgx_ppo_mirror_loss_reduce", 0) == 0 and fus._fused.sym_parts is None
        assert fus.symmetry_loss is None
        params.append([bits(p) for p in fus.actor_critic.parameters()])
    for a, b in zip(*params):
        assert np.array_equal(a, b)
    from legged_gym_amd.rl.actor_critic import ActorCritic
    from legged_gym_amd.rl.ppo import PPO
    for off in (None, {"use_mirror_loss": False, "mirror_loss_coeff": 1.0}):
        fus = PPO(ActorCritic(235, 235, ACT, [512, 256, 128], [512, 256, 128]), device=DEV, symmetry=off)
        assert fus._fused is not None and fus.symmetry is False
        fus.init_storage(N, T, [235], [None], [ACT])
        st = fus.storage
        assert st.symmetry is None and st.observations.shape == (T, N, 235) and st.full("observations") is st.observations
        assert st.observations.untyped_storage().nbytes() == B * 235 * 4
        assert st.actions.untyped_storage().nbytes() == B * ACT * 4 and st.advantages.untyped_storage().nbytes() == B * 4


@pytest.mark.parametrize("switch", ["LGX_PPO_LOSS_BWD", "LGX_PPO_HEAD_IN_LOSS"])
def test_a_plan_without_the_paired_launch_is_refused(gpu, tables, monkeypatch, switch):
    monkeypatch.setenv(switch, "0")
    _, fus = make_sym_pair(pick(tables, 235, None), symmetry=MIRROR)
    before = [p.detach().clone() for p in fus.actor_critic.parameters()]
    for _ in range(2):                                                    # at the first update, and at every later one
        with pytest.raises(ValueError, match=f"use_mirror_loss.*{switch}=0"):
            fus.update()
    for a, b in zip(before, fus.actor_critic.parameters()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- end to end
def test_go1_rough_mirror_end_to_end(gpu, tmp_path):
    from legged_gym_amd.rl.runner import OnPolicyRunner
    from legged_gym_amd.utils.helpers import class_to_dict
    env = make_env("go1_rough_mirror", num_envs=64, device=DEV, backend="lgx")
    cfg = class_to_dict(task_registry.get_cfgs("go1_rough_mirror")[1])
    assert cfg["algorithm"]["symmetry"]["use_mirror_loss"] is True
    torch.manual_seed(0)
    runner = OnPolicyRunner(env, cfg, str(tmp_path), device=DEV)
    st = runner.alg.storage
    assert runner.alg._fused is not None and st.symmetry is not None and st.full("observations").shape[0] == 2 * 24
    runner.alg._fused.lib = spy = _CallCounter(runner.alg._fused.lib)
    runner.learn(2, init_at_random_ep_len=True)
    assert spy.calls.get("lgx_ppo_symmetry_augment", 0) == 2 and spy.calls.get("lgx_ppo_loss_bwd_mirror", 0) == 2 * 5 * 4
    stats = runner.last_iteration_stats
    assert np.isfinite([stats["value_loss"], stats["surrogate_loss"], stats["learning_rate"], stats["symmetry_loss"]]).all()
    assert stats["symmetry_loss"] > 0, stats
    path = tmp_path / "model_2.pt"
    assert path.exists()
    other = OnPolicyRunner(env, cfg, None, device=DEV)
    other.load(str(path))
    for a, b in zip(runner.alg.actor_critic.parameters(), other.alg.actor_critic.parameters()):
        assert torch.equal(a, b)
    assert other.current_learning_iteration == 2
