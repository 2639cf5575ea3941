"""The PPO update of rsl_rl v1.0.x (`PPO.update`; legged_robot_config.py:226-239) as an explicit
forward/backward over flat parameter/gradient buffers — no autograd graph, no per-op launches.

Per minibatch (M rows), no host synchronisation (the stages of `_minibatch_body`):
  inputs: the weight copies of the GEMMs (bf16 limbs / padded, transposed f32) prepared on an
          update's first minibatch, afterwards kept current by the Adam step; the layer-1 input
          rows gathered with K padded to a multiple of abi.GEMM_K_STEP = 32 (once per update)
  forward: lgx_gemm_nt with the bias + ELU epilogue, {actor, critic} batched in one launch
  loss / heads: lgx_ppo_loss_bwd = output layers, log-prob / ratio / clipped surrogate / clipped
          value loss / entropy / KL, the analytic gradient w.r.t. mu, value, std, head biases and
          the output-layer backward; its finalize (in the reduction launch) applies the device-side
          adaptive schedule (data-parallel: lgx_ppo_adapt_lr after the all-reduce the KL rides in)
          (symmetry.use_mirror_loss: lgx_ppo_loss_bwd_mirror in its place, the same launch with the
          mirror term on the minibatch's mirror rows)
  backward: per layer lgx_gemm_tn for dW (split-K, on a second stream) next to lgx_gemm_nt for dA
          with the ELU' epilogue; the bias gradients are column sums from either
  reductions: lgx_reduce_slices*: all split-K and bias partials -> flat gradient
          [data-parallel: the flat gradient + the minibatch KL all-reduced over RCCL, two buckets]
  optimizer step: lgx_adam_clip*: clip_grad_norm_(max_grad_norm) + Adam on the flat buffers
  (hidden widths that are not multiples of 128, or LGX_PPO_GEMM=lib: library GEMMs through torch
   + lgx_bias_act / lgx_elu_bwd_colsum instead of lgx_gemm_nt / lgx_gemm_tn)
Which of these launches a configuration issues is decided in three places: `_switches` reads the
environment, `_policy_plan` takes the policy apart (supported() and __init__ share it), `_alloc`
builds the launch plan for a minibatch size.
The module's nn.Parameters become views of the flat buffer, so state_dict / load_state_dict /
the rollout's fused inference see the updated weights; the optimizer is `FlatAdam`, whose
state_dict has torch.optim.Adam's format (checkpoints stay loadable by upstream tooling).
"""
import ctypes as C
import os
import time
from types import SimpleNamespace

import torch
import torch.nn as nn

from legged_gym_amd.sim import abi


def _switches():
    """The update's environment switches (DESIGN.md 4.5 has the table): the module's only reader
    of os.environ.  Plan switches are taken when the launch plan is built (supported() / __init__,
    or _alloc for a new minibatch size); run switches at the start of every update() /
    gradients() call, for all of its minibatches."""
    env = os.environ.get

    def on(name):
        return env(name, "1") != "0"
    return SimpleNamespace(
        # plan
        gemm=env("LGX_PPO_GEMM", "lgx"),                  # "lgx" | "auto" | "lib"
        split=env("LGX_GEMM_ALGO", "split") != "f32",
        dw_lgx=env("LGX_PPO_DW", "lgx") != "lib",
        splits=env("LGX_PPO_SPLITS"),                     # "s1,s2,..." per layer
        head_in_loss=on("LGX_PPO_HEAD_IN_LOSS"),
        loss_bwd=on("LGX_PPO_LOSS_BWD"),
        tn_colsum=on("LGX_PPO_TN_COLSUM"),
        fused_sq=on("LGX_PPO_FUSED_SQ"),
        fused_recurrent=on("LGX_PPO_FUSED_RECURRENT"),
        # plan (the dW slices' CU fill) and run (dW on the side stream)
        dw_side=on("LGX_PPO_DW_SIDE"),
        # run
        early_reduce=on("LGX_PPO_EARLY_REDUCE"),
        dev_events=on("LGX_PPO_DEV_EVENTS"),
        bind=on("LGX_PPO_BIND"),
        dw1_batched=on("LGX_PPO_DW1_BATCHED"),
        # process-wide
        tuned_gemms=on("LGX_TUNED_GEMMS"),
        native_allreduce=env("LGX_NATIVE_ALLREDUCE", "0") == "1")


class _TunedGemms:
    """The GEMM solution table tuned on MI355X for the PPO-update shapes (torch TunableOp,
    rocBLAS / hipBLASLt solutions; regenerate with tools/tune_gemms.sh), scoped: TunableOp is
    switched on, read-only (no tuning, no recording of untuned shapes), with this table's file
    name, only inside `with` blocks around the update's library GEMMs; every TunableOp setting
    the caller had (enable, tuning, recording, file name) is restored on exit, so other torch GEMMs
    of the process are unaffected.  Shapes not in the table run the library default.
    LGX_TUNED_GEMMS=0 disables."""
    _loaded = None

    def __init__(self):
        self.ok = False
        if not _switches().tuned_gemms:
            return
        import torch.cuda.tunable as tunable
        from legged_gym_amd import LEGGED_GYM_ROOT_DIR
        path = os.path.join(LEGGED_GYM_ROOT_DIR, "resources", "tunableop", "ppo_gemms_gfx950.csv")
        if not os.path.exists(path):
            return
        self.tunable, self.path = tunable, path
        if _TunedGemms._loaded is None:
            saved = self._save()
            self._apply()
            _TunedGemms._loaded = bool(tunable.read_file(path))
            self._restore(saved)
        self.ok = _TunedGemms._loaded

    def _save(self):
        t = self.tunable
        return (t.is_enabled(), t.tuning_is_enabled(), t.record_untuned_is_enabled(), t.get_filename())

    def _apply(self):
        t = self.tunable
        t.enable(True)
        t.tuning_enable(False)
        t.record_untuned_enable(False)
        t.set_filename(self.path, insert_device_ordinal=False)

    def _restore(self, saved):
        t = self.tunable
        enabled, tuning, record, filename = saved
        t.tuning_enable(tuning)
        t.record_untuned_enable(record)
        if filename:
            t.set_filename(filename, insert_device_ordinal=False)
        t.enable(enabled)

    def __enter__(self):
        if self.ok:
            self.saved = self._save()
            self._apply()
        return self

    def __exit__(self, *exc):
        if self.ok:
            self._restore(self.saved)
        return False


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class FlatAdam:
    """torch.optim.Adam (no weight decay, no amsgrad) over one flat parameter buffer, with the
    learning rate and the step counter resident on the device."""

    def __init__(self, params, flat_p, flat_g, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        self.flat_p, self.flat_g = flat_p, flat_g
        self.m = torch.zeros_like(flat_p)
        self.v = torch.zeros_like(flat_p)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=flat_p.device)
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float64, device=flat_p.device)
        self.betas, self.eps = betas, eps
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                  foreach=None, capturable=False, differentiable=False, fused=None)]

    def _views(self, buf):
        base = self.flat_p.data_ptr()
        out = []
        for p in self.params:
            off = (p.data_ptr() - base) // 4
            out.append(buf[off:off + p.numel()].view_as(p))
        return out

    def zero_grad(self, set_to_none=False):
        self.flat_g.zero_()

    def state_dict(self):
        step = float(self.step_dev.item())
        ms, vs = self._views(self.m), self._views(self.v)
        state = {i: {"step": torch.tensor(step), "exp_avg": ms[i].clone(), "exp_avg_sq": vs[i].clone()}
                 for i in range(len(self.params)) if step > 0}
        g = dict(self.param_groups[0])
        g["lr"] = float(self.lr_dev.item())
        g["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, d):
        g = d["param_groups"][0]
        self.lr_dev.fill_(float(g["lr"]))
        self.param_groups[0]["lr"] = float(g["lr"])
        ms, vs = self._views(self.m), self._views(self.v)
        step = 0
        with torch.no_grad():
            for i, st in d["state"].items():
                i = int(i)
                ms[i].copy_(st["exp_avg"])
                vs[i].copy_(st["exp_avg_sq"])
                step = int(float(st["step"]))
        self.step_dev.fill_(step)


def _policy_plan(ac, sw):
    """The policy taken apart for the update, under the plan switches `sw`: the linear layers of
    actor and critic, the hidden widths and which GEMM paths drive them - or None for a policy
    that __init__ + _alloc cannot drive (supported() is exactly this test)."""
    recurrent = bool(getattr(ac, "is_recurrent", False))
    if recurrent and not (sw.fused_recurrent and hasattr(ac, "memory_a") and hasattr(ac, "memory_c")):
        return None   # (LGX_PPO_FUSED_RECURRENT=0: recurrent policies on the autograd update)
    try:
        nets = [list(ac.actor), list(ac.critic)]
    except AttributeError:
        return None
    (la, aa), (lc, acr) = (([m for m in net if isinstance(m, nn.Linear)],
                            [m for m in net if not isinstance(m, nn.Linear)]) for net in nets)
    if not all(isinstance(m, nn.ELU) and m.alpha == 1.0 for m in aa + acr):
        return None
    if len(la) != len(lc) or len(la) < 2 or len(aa) != len(la) - 1 or len(acr) != len(lc) - 1:
        return None
    hidden = [l.out_features for l in la[:-1]]
    L = len(hidden)
    # one lgx_reduce_slices launch takes every gradient block: dW1 (x2 with a privileged critic
    # of another width), dW_2..L, the head dW, and the bias sums of every hidden layer; the
    # weight copies the Adam step maintains: padded W1 (x2) + transposed W_2..L
    sep = la[0].in_features != lc[0].in_features
    jobs = 2 * L + 1 + int(sep)
    mirrors = 2 * L - 1 + int(sep)     # split-bf16 limb copies: W_1 (x2), W_k and W_k^T
    if not (hidden == [l.out_features for l in lc[:-1]] and all(hk % 4 == 0 for hk in hidden) and hidden[-1] <= 1024
            and lc[-1].out_features == 1 and la[-1].out_features <= abi.PPO_MAX_ACTIONS and ac.std.dim() == 1
            and jobs <= abi.MAX_REDUCE_JOBS and mirrors <= abi.MAX_REDUCE_JOBS):
        return None
    # lgx_gemm: the hidden layers on lgx_gemm_nt (LGX_PPO_GEMM "lgx": every forward and dA; "auto":
    # the layer-1 forward and the dA products, library GEMM + lgx_bias_act for the other forwards),
    # else ("lib", or widths off the GEMM's N tile) library GEMMs.  split: its split-bf16 products
    # with pre-split weights, else exact-f32 MFMA with f32 weight copies.  tn: the weight gradients
    # on lgx_gemm_tn (split-bf16 only), else library f32 bmm over row slices
    lgx_gemm = all(hk % abi.GEMM_TILE_N == 0 for hk in hidden) and sw.gemm != "lib"
    if recurrent and not lgx_gemm:
        return None   # (the memories' outputs enter through the padded rows of the lgx_gemm plan only)
    return SimpleNamespace(la=la, lc=lc, hidden=hidden, recurrent=recurrent, lgx_gemm=lgx_gemm,
                           lgx_fwd_layers=set(range(L)) if sw.gemm == "lgx" else {0}, split=sw.split,
                           tn=lgx_gemm and sw.split and sw.dw_lgx)


_UNTRIED = object()   # FusedPPOUpdate._comm before _lgx_comm() has run


class FusedPPOUpdate:
    """Drives the lgx PPO kernels for a standard rsl_rl ActorCritic (identical ELU hidden stacks
    for actor and critic)."""

    SPLITS = 8

    # state created on first use (None / empty until then)
    run = None                                   # the run switches of the current update() / gradients() call
    _side = _ev_in = _ev_out = None              # the backward's second stream and its torch join events
    _dev_ev = _armed = None                      # device join events; the slot bound to the next launch
    _perm_stream = None
    _pin_stats = _pin_lr = _pin_ev = None        # a deferred update's readback
    _comm, _comm_last = _UNTRIED, None           # lgx_comm (None: the torch path); its last collective
    _t_period = _t_count = _t_mb = 0             # time_gemms()
    _t_events = _c_events = ()
    Xall = Xall2 = Xcall = None                  # _gather_all's buffers
    time_augment, augment_events = False, ()     # tools/train_time.py: event pairs around each augment launch
    sym_parts = sym_stat = _pin_sym = None       # mirror loss: per-minibatch partials, the update's mean, its readback
    _sym_slot = 0
    _rec_idx = _mem_ctx = None                   # recurrent minibatches

    @staticmethod
    def supported(ac):
        return _policy_plan(ac, _switches()) is not None

    def __init__(self, ppo):
        from legged_gym_amd.sim import lib as lgxlib
        self.lib = lgxlib.load()
        self.check = lgxlib.check
        self.tuned = _TunedGemms()
        self.ppo = ppo
        ac = ppo.actor_critic
        self.dev = next(ac.parameters()).device
        plan = _policy_plan(ac, _switches())
        if plan is None:
            raise ValueError("FusedPPOUpdate.supported(actor_critic) is False for this policy")
        la, lc = plan.la, plan.lc
        self.hidden, self.recurrent = plan.hidden, plan.recurrent
        self.lgx_gemm, self.lgx_fwd_layers, self.split, self.tn = plan.lgx_gemm, plan.lgx_fwd_layers, plan.split, plan.tn
        self.L = len(la) - 1                       # hidden layers
        self.num_obs = la[0].in_features
        self.num_cobs = lc[0].in_features
        self.A = la[-1].out_features
        # flat layout: layer-major so that {actor, critic} blocks of a layer are adjacent; the layer-1
        # biases right after the layer-1 weights: both come from dW1's lgx_gemm_tn (weights, and the
        # bias gradient from its column sums), so the second data-parallel gradient bucket - what
        # is complete only once dW1 is - is the contiguous prefix [0, nW1)
        order = [la[0].weight, lc[0].weight, la[0].bias, lc[0].bias]
        for k in range(1, self.L + 1):
            order += [la[k].weight, lc[k].weight]
        for k in range(1, self.L + 1):
            order += [la[k].bias, lc[k].bias]
        order.append(ac.std)
        # recurrent policies (ActorCriticRecurrent): the memories' parameters after the heads' (their
        # gradients come from torch autograd through the LSTM / GRU, fed with the heads' input
        # gradient dX = dZ_1 W_1 of the fused backward; the clip norm and Adam cover them too)
        self.mem_params = (list(ac.memory_a.parameters()) + list(ac.memory_c.parameters())) if self.recurrent else []
        order += self.mem_params
        n = sum(p.numel() for p in order)
        self.flat_p = torch.zeros(n, device=self.dev)
        # gradient buffer + one trailing slot: the minibatch KL rides in the same all-reduce as the
        # gradient when data-parallel (one collective per minibatch)
        self.g_comm = torch.zeros(n + 1, device=self.dev)
        self.flat_g = self.g_comm[:n]
        self.off = {}
        off = 0
        with torch.no_grad():
            for p in order:
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.data.reshape(-1))
                self.off[id(p)] = off
                p.data = self.flat_p[off:off + k].view_as(p)
                p.grad = self.flat_g[off:off + k].view_as(p)
                off += k
        self.n = n
        self.nW1 = self.off[id(la[1].weight)]   # end of the {actor, critic} layer-1 weight + bias blocks
        self.bucketed = False                     # (last minibatch: two all-reduce buckets)
        self.la, self.lc = la, lc
        self.W = []    # per layer k < L: stacked [2, out, in] weight view (k >= 1) or per-net views (k == 0)
        for k in range(self.L + 1):
            o = self.off[id(la[k].weight)]
            if k == 0 or k == self.L:
                self.W.append((la[k].weight, lc[k].weight))
            else:
                self.W.append(self.flat_p[o:o + 2 * la[k].weight.numel()].view(2, *la[k].weight.shape))
        self.Wg = [self.off[id(la[k].weight)] for k in range(self.L + 1)]
        if self.num_obs == self.num_cobs:
            o = self.Wg[0]
            self.W1s = self.flat_p[o:o + 2 * la[0].weight.numel()].view(2, *la[0].weight.shape)
        self.bo = [self.off[id(la[k].bias)] for k in range(self.L + 1)]
        self.std_off = self.off[id(ac.std)]
        params = list(ac.parameters())
        self.optimizer = FlatAdam(params, self.flat_p, self.flat_g, ppo.learning_rate)
        self.gemm_dw = {}   # layer -> lgx_gemm_tn argument blocks (filled by _build_gemm_plan)
        self.colsum = {}    # layer -> dW's column-sum partials (the bias gradient; _build_gemm_plan)
        self.norm_parts = torch.zeros(256, device=self.dev)
        self._mirrors_valid = False
        self.stats = torch.zeros(3, device=self.dev)
        self._pending = None      # a deferred update's readback (update(defer=True) -> resolve())
        self.M = None

    # ------------------------------------------------------------------ buffers
    def _alloc(self, M):
        """Buffers and the launch plan for minibatches of M rows, under the plan switches read
        here (kept until M changes)."""
        if self.M == M:
            return
        dev, h, A = self.dev, self.hidden, self.A
        sw = _switches()
        self.M = M
        # split-K row slices of each layer's dW GEMM (library bmm over slices, partials reduced in
        # lgx_reduce_slices): enough output tiles to fill the CUs (half of them when dW runs on the
        # side stream next to the dA GEMMs). LGX_PPO_SPLITS="s1,s2,..." per layer
        want = [int(x) for x in sw.splits.split(",")] if sw.splits else []
        fill = 0.5 if sw.dw_side else 1.0
        self.Sk = []
        for k in range(self.L):
            sk = want[k] if k < len(want) else (self._tn_slices(h[k], h[k - 1] if k else self.num_obs, M, fill=fill)
                                                if self.tn else self.SPLITS)
            self.Sk.append(sk if sk > 0 and M % sk == 0 else 1)
        self.S = self.Sk[0]
        sep = self._separate_critic_obs()
        if self.lgx_gemm:   # K of layer 1 padded to the GEMM's K step with zero columns
            ks = abi.GEMM_K_STEP
            self.Kp, self.Kcp = -(-self.num_obs // ks) * ks, -(-self.num_cobs // ks) * ks
            self.Xp = torch.zeros(M, self.Kp, device=dev)
            self.X = self.Xp[:, :self.num_obs]
            self.Xcp = torch.zeros(M, self.Kcp, device=dev) if sep else None
            self.Xc = self.Xcp[:, :self.num_cobs] if sep else None
        else:
            self.X = torch.empty(M, self.num_obs, device=dev)
            self.Xc = torch.empty(M, self.num_cobs, device=dev) if sep else None
        self.Y = [torch.empty(2, M, hk, device=dev) for hk in h]
        self.D = [torch.empty(2, M, hk, device=dev) for hk in h[:-1]]
        self.MU = torch.empty(M, A, device=dev)
        self.V = torch.empty(M, 1, device=dev)
        self.dMU = torch.empty(M, A, device=dev)
        self.dV = torch.empty(M, device=dev)
        Sk = self.Sk
        # layer-1 dW partials: one [2, S, h0, K] block (one input for both networks), or (actor,
        # critic) blocks when the critic reads inputs of its own (privileged observations, of any
        # width; a recurrent policy's two memory outputs)
        p0 = (torch.empty(2, Sk[0], h[0], self.num_obs, device=dev) if self.num_cobs == self.num_obs and not sep else
              (torch.empty(Sk[0], h[0], self.num_obs, device=dev), torch.empty(Sk[0], h[0], self.num_cobs, device=dev)))
        self.P = [p0] + \
                 [torch.empty(2 * Sk[k], h[k], h[k - 1], device=dev) for k in range(1, self.L)]
        # output layers evaluated inside the loss call (no head GEMM launches) when they fit its LDS;
        # with them, loss + output-layer backward in one launch (lgx_ppo_loss_bwd, its loss finalize
        # in the reduction launch) unless LGX_PPO_LOSS_BWD=0
        H = h[-1]
        self.head_in_loss = sw.head_in_loss and H % 16 == 0 and (A + 1) * H * 4 <= 65536
        lay = (C.c_int64 * 3)()
        self.check(self.lib.lgx_ppo_loss_bwd_layout(M, A, H, lay), "loss_bwd_layout")
        self.loss_bwd = self.head_in_loss and lay[2] <= 96 * 1024 and sw.loss_bwd
        if self.ppo.mirror_loss_coeff is not None and not self.loss_bwd:
            # the mirror term lives in the paired form of that launch alone: never train without it
            self.M = None
            why = ("LGX_PPO_LOSS_BWD=0" if not sw.loss_bwd else "LGX_PPO_HEAD_IN_LOSS=0" if not sw.head_in_loss else
                   f"a head of {A} actions on {H} hidden units does not fit lgx_ppo_loss_bwd's LDS")
            raise ValueError("symmetry.use_mirror_loss needs the fused loss / output-layer launch "
                             f"(lgx_ppo_loss_bwd_mirror), which this plan does not run: {why}")
        if self.loss_bwd:
            self.loss_parts = torch.empty(int(lay[0]), device=dev)
            self.head_parts = torch.empty(int(lay[1]), device=dev)
        else:
            self.loss_parts = torch.empty(int(self.lib.lgx_ppo_loss_partials_floats(M, A)), device=dev)
            self.head_parts = torch.empty(int(self.lib.lgx_head_bwd_partials_floats(M, A, H)), device=dev)
        self.gemm_dw, self.colsum = {}, {}
        if self.lgx_gemm:
            self.col_parts = [torch.empty(int(self.lib.lgx_gemm_partials_floats(M, hk, 2)), device=dev)
                              for hk in h[:-1]]
            self._build_gemm_plan(sw)
        else:
            self.col_parts = [torch.empty(int(self.lib.lgx_colsum_partials_floats(M, hk, 2)), device=dev)
                              for hk in h[:-1]]
        self._build_reduce_jobs(sw)

    @staticmethod
    def _tn_slices(R, Cc, M, cus=256, fill=1.0):
        """Row slices of one lgx_gemm_tn launch: the fewest (>= 8, powers of 2) that give a
        fraction `fill` of the CUs an output tile (R/128 x ceil(Cc/128) tiles per slice and
        network) with 32-row multiples."""
        tiles = (R // (256 if R % 256 == 0 else 128)) * (-(-Cc // 128)) * 2   # lgx_gemm_tn tile rows
        s = 8
        while tiles * s < cus * fill and M % (2 * s * 32) == 0:
            s *= 2
        while s > 1 and M % (s * 32):   # small minibatches: fewer slices of 32-row multiples
            s //= 2
        return s

    def _build_gemm_plan(self, sw):
        """Fixed argument blocks of every lgx_gemm_nt / lgx_copy2d launch of a minibatch (the
        buffers do not move, so a minibatch issues the prepared structs)."""
        M, h, L, dev = self.M, self.hidden, self.L, self.dev
        fp = self.flat_p
        f4 = 4
        shared = self.Xcp is None and self.num_obs == self.num_cobs
        copies = []

        def copy(src_ptr, dst, rows, cols, batch, transpose, src_ld, dst_ld, limbs=0):
            j = abi.LgxCopy2dJob()
            j.src, j.dst = src_ptr, dst.data_ptr()
            j.src_ld, j.src_bs = src_ld, rows * cols
            j.dst_ld, j.dst_bs = dst_ld, (cols if transpose else rows) * dst_ld
            j.rows, j.cols, j.batch, j.transpose = rows, cols, batch, int(transpose) | limbs
            copies.append(j)
        w1 = fp.data_ptr() + f4 * self.Wg[0]
        nl = [None] * (L + 1)   # split-bf16: limb copies of W_1 / W_k (forward) and W_k^T (backward dA)
        nlt = [None] * (L + 1)
        if self.split:
            # the B operands pre-split into bf16 limbs (lgx_split_bf16 before an update's first
            # minibatch, then kept current by the Adam step's limb mirrors: transpose bit 1)
            def limbs(src_ptr, rows, cols, batch, transpose):
                nout, kout = (cols, rows) if transpose else (rows, cols)
                ld = int(self.lib.lgx_split_bf16_elems(1, kout))
                buf = torch.zeros(batch * nout * ld, dtype=torch.int16, device=dev)
                copy(src_ptr, buf, rows, cols, batch, transpose, cols, ld, limbs=2)
                return buf
            if shared:
                nl[0] = (limbs(w1, h[0], self.num_obs, 2, False),)
            else:
                nl[0] = (limbs(w1, h[0], self.num_obs, 1, False),
                         limbs(w1 + f4 * h[0] * self.num_obs, h[0], self.num_cobs, 1, False))
            for k in range(1, L):
                wk = fp.data_ptr() + f4 * self.Wg[k]
                nl[k] = limbs(wk, h[k], h[k - 1], 2, False)
                nlt[k] = limbs(wk, h[k], h[k - 1], 2, True)
            self.limb_bufs = (nl, nlt)
        else:
            if shared:
                self.W1p = torch.zeros(2, h[0], self.Kp, device=dev)
                copy(w1, self.W1p, h[0], self.num_obs, 2, False, self.num_obs, self.Kp)
            else:
                self.W1p = torch.zeros(h[0], self.Kp, device=dev)
                self.W1pc = torch.zeros(h[0], self.Kcp, device=dev)
                copy(w1, self.W1p, h[0], self.num_obs, 1, False, self.num_obs, self.Kp)
                copy(w1 + f4 * h[0] * self.num_obs, self.W1pc, h[0], self.num_cobs, 1, False, self.num_cobs, self.Kcp)
            self.WT = [None]
            for k in range(1, L):   # W_k [2, h_k, h_{k-1}] -> W_k^T [2, h_{k-1}, h_k]
                wt = torch.empty(2, h[k - 1], h[k], device=dev)
                copy(fp.data_ptr() + f4 * self.Wg[k], wt, h[k], h[k - 1], 2, True, h[k - 1], h[k])
                self.WT.append(wt)
        if len(copies) > abi.MAX_REDUCE_JOBS:
            raise RuntimeError("too many weight-preparation jobs for one launch")
        self.copy_jobs = (abi.LgxCopy2dJob * len(copies))(*copies)
        algo = abi.GEMM_ALGO_SPLIT_BF16 if self.split else abi.GEMM_ALGO_F32

        def gemm(A, lda, sa, B, ldb, sb, C, N, K, batch, epi, bias=None, Y=None, parts=None, Bs=None):
            g = abi.LgxGemmArgs()
            g.M, g.N, g.K, g.batch, g.epi = M, N, K, batch, epi
            g.A, g.lda, g.sa = A, lda, sa
            g.B, g.ldb, g.sb = B, ldb, sb
            g.C, g.ldc, g.sc = C.data_ptr(), N, M * N
            g.bias = bias
            g.Y = Y.data_ptr() if Y is not None else None
            g.partials = parts.data_ptr() if parts is not None else None
            g.algo = algo
            g.Bs = Bs.data_ptr() if Bs is not None else None
            return g
        fwd = [[]]
        b0 = fp.data_ptr() + f4 * self.bo[0]
        w1p = None if self.split else self.W1p.data_ptr()
        if shared:   # one input for both networks: batch stride 0
            fwd[0].append(gemm(self.Xp.data_ptr(), self.Kp, 0, w1p, self.Kp, h[0] * self.Kp, self.Y[0],
                               h[0], self.Kp, 2, abi.GEMM_BIAS_ELU, bias=b0, Bs=nl[0][0] if self.split else None))
        else:
            fwd[0].append(gemm(self.Xp.data_ptr(), self.Kp, 0, w1p, self.Kp, 0, self.Y[0][0], h[0],
                               self.Kp, 1, abi.GEMM_BIAS_ELU, bias=b0, Bs=nl[0][0] if self.split else None))
            xc = self.Xcp if self.Xcp is not None else self.Xp
            fwd[0].append(gemm(xc.data_ptr(), self.Kcp, 0, None if self.split else self.W1pc.data_ptr(), self.Kcp, 0,
                               self.Y[0][1], h[0], self.Kcp, 1, abi.GEMM_BIAS_ELU, bias=b0 + f4 * h[0],
                               Bs=nl[0][1] if self.split else None))
        for k in range(1, L):
            fwd.append(gemm(self.Y[k - 1].data_ptr(), h[k - 1], M * h[k - 1], fp.data_ptr() + f4 * self.Wg[k], h[k - 1],
                            h[k] * h[k - 1], self.Y[k], h[k], h[k - 1], 2, abi.GEMM_BIAS_ELU,
                            bias=fp.data_ptr() + f4 * self.bo[k], Bs=nl[k]))
        self.gemm_fwd = fwd
        # algorithmic K of each launch (layer 1: the unpadded input width) for the bench's roofline
        self.k_alg = {id(g): k for g, k in zip(fwd[0], [self.num_obs, self.num_cobs])}
        # weight gradients (lgx_gemm_tn): dW_k = dZ_k^T Y_{k-1} over Sk row slices into P[k]
        if self.tn:
            def tn(A, lda, sa, B, ldb, sb, Cp, R, Cc, S, batch):
                t = abi.LgxGemmTnArgs()
                t.M, t.R, t.Cc, t.slices, t.batch = M, R, Cc, S, batch
                t.A, t.lda, t.sa = A, lda, sa
                t.B, t.ldb, t.sb = B, ldb, sb
                t.C, t.ldc = Cp, Cc
                return t
            tn_ok = [M % (self.Sk[k] * 32) == 0 for k in range(L)]   # else the library bmm (rows % 32)
            for k in range(L - 1, 0, -1):
                if not tn_ok[k]:
                    continue
                dz = self.Y[L - 1] if k == L - 1 else self.D[k]
                self.gemm_dw[k] = [tn(dz.data_ptr(), h[k], M * h[k], self.Y[k - 1].data_ptr(), h[k - 1], M * h[k - 1],
                                      self.P[k].data_ptr(), h[k], h[k - 1], self.Sk[k], 2)]
            # layer 1: B = the minibatch's padded input rows (pointer set per minibatch); the padding
            # columns up to the next multiple of 128 must exist in the rows
            if tn_ok[0] and self.Kp >= -(-self.num_obs // 128) * 128 and (
                    self.Xcp is None or self.Kcp >= -(-self.num_cobs // 128) * 128):
                d0 = self.D[0]
                if isinstance(self.P[0], tuple):     # privileged critic inputs: one launch per network
                    self.gemm_dw[0] = [tn(d0[0].data_ptr(), h[0], 0, 0, self.Kp, 0, self.P[0][0].data_ptr(), h[0],
                                          self.num_obs, self.Sk[0], 1),
                                       tn(d0[1].data_ptr(), h[0], 0, 0, self.Kcp, 0, self.P[0][1].data_ptr(), h[0],
                                          self.num_cobs, self.Sk[0], 1)]
                else:                                # one input for both networks: batch stride 0
                    self.gemm_dw[0] = [tn(d0.data_ptr(), h[0], M * h[0], 0, self.Kp, 0, self.P[0].data_ptr(), h[0],
                                          self.num_obs, self.Sk[0], 2)]
        # bias gradients db_k of the hidden layers below the last: the column sums of dZ_k, taken by
        # dW_k's lgx_gemm_tn from the rows it stages anyway (per-slice partials, reduced with the
        # weight gradients); the dA GEMM producing dZ_k then runs the plain ELU' epilogue.
        # Layers whose dW is not on lgx_gemm_tn keep the ELU' + column-sum epilogue.
        if self.split and sw.tn_colsum:
            for k in range(L - 1):
                if k not in self.gemm_dw:
                    continue
                cs = torch.empty(2, self.Sk[k], h[k], device=dev)
                self.colsum[k] = cs
                for z, t in enumerate(self.gemm_dw[k]):   # (batch 2, or one launch per network)
                    t.colsum = cs.data_ptr() + 4 * z * self.Sk[k] * h[k]
        bwd = {}
        for k in range(L - 1, 0, -1):   # dZ_{k-1} = (dZ_k W_k) * elu'(Y_{k-1}); dZ_{L-1} lives in Y[L-1]
            dz = self.Y[L - 1] if k == L - 1 else self.D[k]
            plain = (k - 1) in self.colsum
            bwd[k] = gemm(dz.data_ptr(), h[k], M * h[k], None if self.split else self.WT[k].data_ptr(), h[k],
                          h[k - 1] * h[k], self.D[k - 1], h[k - 1], h[k], 2,
                          abi.GEMM_DELU if plain else abi.GEMM_DELU_COLSUM, Y=self.Y[k - 1],
                          parts=None if plain else self.col_parts[k - 1], Bs=nlt[k])
        self.gemm_bwd = bwd

    def _separate_critic_obs(self):
        if self.recurrent:   # the heads' inputs are the two memories' outputs
            return True
        st = self.ppo.storage
        return st is not None and st.privileged_observations is not None

    def _build_reduce_jobs(self, sw):
        M, S, h, A = self.M, self.S, self.hidden, self.A
        g = self.flat_g
        jobs = []

        def job(src, dst_off, n, count, job_stride, slices, slice_stride, dst_stride):
            j = abi.LgxReduceJob()
            j.src = src.data_ptr()
            j.dst = g.data_ptr() + 4 * dst_off
            j.n, j.count, j.job_stride, j.slices, j.slice_stride, j.dst_stride = n, count, job_stride, slices, \
                slice_stride, dst_stride
            jobs.append(j)
        n1 = h[0] * self.num_obs
        Sk = self.Sk
        if isinstance(self.P[0], tuple):                                             # dW1 actor, critic
            n1c = h[0] * self.num_cobs
            job(self.P[0][0], self.Wg[0], n1, 1, 0, Sk[0], n1, 0)
            job(self.P[0][1], self.Wg[0] + n1, n1c, 1, 0, Sk[0], n1c, 0)
        else:
            job(self.P[0], self.Wg[0], n1, 2, Sk[0] * n1, Sk[0], n1, n1)            # dW1 (actor, critic)
        colsum = self.colsum
        if 0 in colsum:   # db_1 from dW1's column sums: complete with dW1
            job(colsum[0], self.bo[0], h[0], 2, Sk[0] * h[0], Sk[0], h[0], h[0])
        elif self.L > 1:
            # db_1 from the dA_1 GEMM's ELU' + column-sum partials (dW1 not on lgx_gemm_tn: e.g. 48
            # observations, whose padded rows are narrower than dW1's 128-column tiles).  dA_1 runs on
            # the main stream after the side stream's last join, so this job goes with dW1's: in the
            # side stream's early reduction it would read the partials before dA_1 wrote them
            cchunks = self.col_parts[0].numel() // (2 * h[0])
            job(self.col_parts[0], self.bo[0], 2 * h[0], 1, 0, cchunks, 2 * h[0], 0)
        n_dw1 = len(jobs)   # (the layer-1 jobs come first: the rest can be reduced before dW1 is done)
        for k in range(1, self.L):
            nk = h[k] * h[k - 1]
            job(self.P[k], self.Wg[k], nk, 2, Sk[k] * nk, Sk[k], nk, nk)            # dW_k stacked
        nh = (A + 1) * h[-1] + 2 * h[-1]
        hchunks = self.head_parts.numel() // nh                                     # per-chunk partial rows
        job(self.head_parts, self.Wg[self.L], (A + 1) * h[-1], 1, 0, hchunks, nh, 0)  # dW head (actor | critic)
        hp_b = self.head_parts[(A + 1) * h[-1]:]
        job(hp_b, self.bo[self.L - 1], 2 * h[-1], 1, 0, hchunks, nh, 0)              # db of the last hidden layer
        for k in range(1, self.L - 1):   # (db_1 is with the layer-1 jobs above)
            if k in colsum:                                                          # db_k from dW_k's column sums
                job(colsum[k], self.bo[k], h[k], 2, Sk[k] * h[k], Sk[k], h[k], h[k])
                continue
            cchunks = self.col_parts[k].numel() // (2 * h[k])
            job(self.col_parts[k], self.bo[k], 2 * h[k], 1, 0, cchunks, 2 * h[k], 0)  # db_k
        if len(jobs) > abi.MAX_REDUCE_JOBS:
            raise RuntimeError("too many reduction jobs for one launch")
        self.jobs = (abi.LgxReduceJob * len(jobs))(*jobs)
        self.njobs = len(jobs)
        self.jobs_dw1 = (abi.LgxReduceJob * n_dw1)(*jobs[:n_dw1])
        self.jobs_rest = (abi.LgxReduceJob * (len(jobs) - n_dw1))(*jobs[n_dw1:])
        # every input of jobs_rest comes from the side stream's dW launches (partials, column sums)
        # or from the main stream before the side stream's first join (loss): the early reduction
        # then needs no join after the dA GEMMs (a db_k from a dA epilogue, k >= 2, needs it)
        self.rest_on_side = all(k in colsum for k in range(1, self.L - 1))
        # the clip norm's sums of squares written by the reduction launches themselves
        # (lgx_reduce_slices_sq; single-process updates with the fused loss)
        self.fused_sq = self.lgx_gemm and self.loss_bwd and not self.recurrent and sw.fused_sq
        if self.fused_sq:
            blocks = self.lib.lgx_reduce_slices_blocks
            self.nsq_rest = int(blocks(self.jobs_rest, len(self.jobs_rest), 1)) if len(self.jobs_rest) else 0
            self.nsq_dw1 = int(blocks(self.jobs_dw1, len(self.jobs_dw1), 0))
            self.nsq_all = int(blocks(self.jobs, self.njobs, 1))
            if min(self.nsq_rest, self.nsq_dw1, self.nsq_all) < 0:
                raise RuntimeError("lgx_reduce_slices_blocks failed")
            self.sq_parts = torch.zeros(max(self.nsq_rest + self.nsq_dw1, self.nsq_all, 1), device=self.dev)

    # ------------------------------------------------------------------ update
    @torch.no_grad()
    def update(self, defer=False):
        """One PPO update (rsl_rl PPO.update).  Returns (mean value loss, mean surrogate loss) after
        reading the statistics and the adapted learning rate back (one host synchronisation).
        defer=True returns None right after issuing: the readback goes to pinned host memory behind
        an event and resolve() - called by the next update() or by the caller - applies it, so the
        host can issue the next rollout while this update still runs."""
        self.resolve()   # (a previous deferred update finished long before this one is issued)
        if self.recurrent:
            return self._update_recurrent(defer)
        t_issue = time.perf_counter()
        ppo = self.ppo
        nmb = ppo.num_mini_batches
        B = ppo.storage.num_transitions_per_env * ppo.storage.num_envs
        M = B // nmb
        # symmetry augmentation / mirror loss: M real rows + their M mirrors per minibatch through the
        # same kernels (the mirror loss alone: the PPO terms over the real rows, lgx_ppo_loss_bwd_mirror's ppo_rows)
        sym = ppo.storage.symmetry is not None
        Mr = 2 * M if sym else M
        stream = self._begin_update(Mr)
        if sym:
            self.augment(stream)
        # rsl_rl's permutation, drawn on a second stream (the generator's offset is taken at issue:
        # the same permutation on any stream): its sort chain of small launches runs next to the
        # rollout's last steps / GAE still queued on this stream instead of after them
        main = torch.cuda.current_stream(self.dev)
        if self._perm_stream is None:
            self._perm_stream = torch.cuda.Stream(self.dev)
        with torch.cuda.stream(self._perm_stream):
            indices = torch.randperm(nmb * M, requires_grad=False, device=self.dev)
        main.wait_stream(self._perm_stream)
        indices.record_stream(main)
        if sym:   # minibatch i: perm[iM:(i+1)M], then the same rows' mirrors (row B + r mirrors row r)
            indices = torch.stack((indices.view(nmb, M), indices.view(nmb, M) + B), 1).reshape(-1)
        obs, cobs, storage = self._storage_views()
        args = self._loss_args(storage)
        # rsl_rl draws ONE permutation per update and every epoch walks the same minibatches, so
        # the padded layer-1 inputs are gathered once (one launch over all rows) and a minibatch
        # reads its contiguous slice: no per-minibatch gather
        xs = self._gather_all(indices, obs, cobs, nmb * Mr, stream) if self.lgx_gemm else [None] * nmb
        for _ in range(ppo.num_learning_epochs):
            for i in range(nmb):
                self._minibatch(indices[i * Mr:(i + 1) * Mr], obs, cobs, args, stream, xs=xs[i])
        self.host_issue_s = time.perf_counter() - t_issue   # host time to issue every launch (tools/host_overhead.py)
        return self._finish(ppo.num_learning_epochs * nmb, defer)

    def _begin_update(self, M, reset=True):
        """What every update() / gradients() call starts with: the plan for minibatches of M rows,
        the run switches (held for all of the call's minibatches), and - reset - the learning rate
        and statistics of a new update.  Returns the current stream's handle."""
        self._alloc(M)
        sw, ppo = _switches(), self.ppo
        device_events = sw.dev_events and ppo.dist is None
        self.run = SimpleNamespace(side_on=self.tn and sw.dw_side, early_reduce=sw.early_reduce,
                                   device_events=device_events, bind=device_events and sw.bind,
                                   dw1_batched=sw.dw1_batched)
        self._mirrors_valid = False      # parameters may have changed since the last update
        if reset:
            # (fixed schedule: lr_dev keeps the optimizer's lr, i.e. a checkpoint's after
            # load_state_dict, as torch.optim.Adam's param_groups do)
            if ppo.desired_kl is not None and ppo.schedule == "adaptive":
                self.optimizer.lr_dev.fill_(ppo.learning_rate)
            self.stats.zero_()
        self._sym_slot = 0
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _storage_views(self):
        """(obs, privileged obs or None, the loss kernel's seven storage arrays), flat over the
        T x N transitions - with symmetry augmentation over 2 T x N rows: the transitions, then their
        mirror images (augment())."""
        st = self.ppo.storage
        B = st.num_transitions_per_env * st.num_envs * (2 if st.symmetry is not None else 1)
        obs = st.full("observations").view(B, -1)
        cobs = st.full("privileged_observations").view(B, -1) if st.privileged_observations is not None else None
        return obs, cobs, dict(actions=st.full("actions").view(B, -1), old_logp=st.full("actions_log_prob").view(B),
                               old_mu=st.full("mu").view(B, -1), old_sigma=st.full("sigma").view(B, -1),
                               advantages=st.full("advantages").view(B), target_values=st.full("values").view(B),
                               returns=st.full("returns").view(B))

    def augment(self, stream=None, src_row=0, dst_row=None):
        """lgx_ppo_symmetry_augment on the storage: rows [dst_row, dst_row + B) of every array a
        minibatch reads written from rows [src_row, src_row + B) through the storage's mirror tables
        (B = T x N; by default the mirror half from the real half, once per update)."""
        st = self.ppo.storage
        if st.symmetry is None:
            raise ValueError("augment(): the storage has no symmetry tables")
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        B = st.num_transitions_per_env * st.num_envs
        a = abi.LgxSymmetryArgs()
        a.rows, a.src_row, a.dst_row = B, src_row, B if dst_row is None else dst_row
        a.num_obs, a.num_actions = st.full("observations").shape[-1], st.full("actions").shape[-1]
        for name in ("observations", "actions", "mu", "sigma", "actions_log_prob", "advantages", "values", "returns"):
            setattr(a, name, st.full(name).data_ptr())
        tab = st.symmetry
        a.obs_perm, a.obs_sign = tab["obs"][0].data_ptr(), tab["obs"][1].data_ptr()
        a.act_perm, a.act_sign = tab["actions"][0].data_ptr(), tab["actions"][1].data_ptr()
        if st.privileged_observations is not None:
            a.num_cobs = st.full("privileged_observations").shape[-1]
            a.privileged_observations = st.full("privileged_observations").data_ptr()
            a.cobs_perm, a.cobs_sign = tab["critic_obs"][0].data_ptr(), tab["critic_obs"][1].data_ptr()
        ev = None
        if self.time_augment:   # (tools/train_time.py: the launch's own time, read after the run)
            ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev[0].record()
        self.check(self.lib.lgx_ppo_symmetry_augment(C.byref(a), stream), "lgx_ppo_symmetry_augment")
        if ev:
            ev[1].record()
            self.augment_events = (*self.augment_events, ev)

    def _finish(self, n, defer):
        """The update's readback (statistics, adapted learning rate) over its n minibatches: now, or
        deferred to pinned memory behind an event (resolve())."""
        mirror = self.ppo.mirror_loss_coeff is not None
        if mirror:
            self._reduce_symmetry_loss(n)
        if not defer:
            return self._apply_readback(self.stats.tolist(), float(self.optimizer.lr_dev.item()), n,
                                        float(self.sym_stat.item()) if mirror else None)
        if self._pin_stats is None:
            self._pin_stats = torch.empty(self.stats.shape, dtype=self.stats.dtype).pin_memory()
            self._pin_lr = torch.empty(1, dtype=self.optimizer.lr_dev.dtype).pin_memory()
            self._pin_ev = torch.cuda.Event()
        if mirror:
            if self._pin_sym is None:
                self._pin_sym = torch.empty(1, dtype=self.sym_stat.dtype).pin_memory()
            self._pin_sym.copy_(self.sym_stat, non_blocking=True)
        self._pin_stats.copy_(self.stats, non_blocking=True)
        self._pin_lr.copy_(self.optimizer.lr_dev.view(1), non_blocking=True)
        self._pin_ev.record(torch.cuda.current_stream(self.dev))
        self._pending = n
        return None

    # ------------------------------------------------------------------ recurrent policies
    def _rec_rows(self, i, T, N, envs):
        """Storage rows of recurrent minibatch i in the heads' row order (t-major over the envs
        [i envs, (i + 1) envs): the unpadded memory output [T, envs, H] flattened)."""
        cache = self._rec_idx
        if cache is None or cache[0] != (T, N, envs):
            cache = ((T, N, envs), {})
            self._rec_idx = cache
        if i not in cache[1]:
            t = torch.arange(T, device=self.dev, dtype=torch.int64)[:, None] * N
            cache[1][i] = (t + i * envs + torch.arange(envs, device=self.dev, dtype=torch.int64)[None, :]).reshape(-1)
        return cache[1][i]

    def _update_recurrent(self, defer):
        """rsl_rl PPO.update for ActorCriticRecurrent (reccurent_mini_batch_generator: minibatches of
        whole envs in order, padded trajectories, the memories' saved first-step states).  Per
        minibatch the LSTM / GRU runs forward on torch with autograd (the heads' inputs), the heads
        run the fused forward / loss / backward of a feed-forward policy on those inputs, and
        _memory_backward carries dX = dZ_1 W_1 back through the memories into the flat gradient
        before the clip norm and Adam."""
        t_issue = time.perf_counter()
        ppo, ac = self.ppo, self.ppo.actor_critic
        st = ppo.storage
        T, N = st.num_transitions_per_env, st.num_envs
        nmb = ppo.num_mini_batches
        envs = N // nmb
        M = T * envs
        stream = self._begin_update(M)
        args = self._loss_args(self._storage_views()[2])
        H = self.num_obs
        k = 0
        for (obs_b, cobs_b, _a, _v, _adv, _r, _lp, _mu, _sg, hid_b, masks_b) in \
                st.reccurent_mini_batch_generator(nmb, ppo.num_learning_epochs):
            i = k % nmb
            k += 1
            with torch.enable_grad():
                xa = ac.memory_a(obs_b, masks_b, hid_b[0])       # [T, envs, H]
                xc = ac.memory_c(cobs_b, masks_b, hid_b[1])
            xs = []
            for x, pad in ((xa, self.Xp), (xc, self.Xcp)):
                x2 = x.detach().reshape(M, H)
                if pad.shape[1] == H and x2.is_contiguous() and x2.data_ptr() % 16 == 0:
                    xs.append(x2)
                else:                              # (K padded to the GEMM step: zero columns stay)
                    pad[:, :H].copy_(x2)
                    xs.append(pad)
            self._mem_ctx = (xa, xc)
            self._mem_xs = xs      # (the heads' input rows stay referenced until the next minibatch)
            self._minibatch(self._rec_rows(i, T, N, envs), None, None, args, stream, xs=(xs[0], xs[1]))
            self._mem_ctx = None
        self.host_issue_s = time.perf_counter() - t_issue
        return self._finish(ppo.num_learning_epochs * nmb, defer)

    def _memory_backward(self):
        """The memories' gradients of a recurrent minibatch: dX = dZ_1 W_1 per network (the heads'
        input gradient; dZ_1 from the fused backward), then torch autograd through the LSTM / GRU
        forward of this minibatch, written into the memories' blocks of the flat gradient (every
        other block is complete: this runs after the reductions, on the update's stream)."""
        if self._mem_ctx is None:
            return
        xa, xc = self._mem_ctx
        dz1 = self.D[0] if self.L > 1 else self.Y[self.L - 1]        # [2, M, h1]
        wa, wc = self.W[0]                                           # [h1, H] each
        dxa = torch.mm(dz1[0], wa).view_as(xa)
        dxc = torch.mm(dz1[1], wc).view_as(xc)
        with torch.enable_grad():
            grads = torch.autograd.grad([xa, xc], self.mem_params, grad_outputs=[dxa, dxc], allow_unused=True)
        for p, g in zip(self.mem_params, grads):
            if g is None:
                p.grad.zero_()
            else:
                p.grad.copy_(g)

    def _apply_readback(self, s, lr, n, sym=None):
        ppo = self.ppo
        if ppo.desired_kl is not None and ppo.schedule == "adaptive":
            ppo.learning_rate = lr
        self.optimizer.param_groups[0]["lr"] = lr
        self.last_losses = (s[2] / n, s[1] / n)
        if sym is not None:   # the mirror loss's mean symmetry loss
            ppo.symmetry_loss = sym
        return self.last_losses

    def _mirror_args(self):
        """What lgx_ppo_loss_bwd_mirror takes beside the loss arguments, for the next minibatch of this
        update() / gradients() call: (action perm, sign, coeff, ppo_rows, symmetry partials) - the
        storage's action table, the PPO terms over all rows (augmentation) or the real half, and the
        minibatch's own slot of symmetry partials (summed once, by _reduce_symmetry_loss)."""
        ppo, M = self.ppo, self.M
        per = int(self.lib.lgx_ppo_mirror_partials_floats(M))
        slots = max(ppo.num_learning_epochs * ppo.num_mini_batches, 1)
        if self.sym_parts is None or self.sym_parts.numel() != slots * per:
            self.sym_parts = torch.zeros(slots * per, device=self.dev)
            self.sym_stat = torch.zeros(1, device=self.dev)
        if self._sym_slot >= slots:
            raise RuntimeError("more minibatches than symmetry-loss slots in one update")
        perm, sign = ppo.storage.symmetry["actions"]
        parts = C.c_void_p(self.sym_parts.data_ptr() + 4 * self._sym_slot * per)
        self._sym_slot += 1
        return _vp(perm), _vp(sign), ppo.mirror_loss_coeff, M if ppo.symmetry_augment else M // 2, parts

    def _reduce_symmetry_loss(self, n):
        """sym_stat = the mean over the call's n minibatches of L_sym (each a mean over M / 2 rows x A)."""
        per = int(self.lib.lgx_ppo_mirror_partials_floats(self.M))
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.check(self.lib.lgx_ppo_mirror_loss_reduce(_vp(self.sym_parts), n * per, 1.0 / (n * (self.M // 2) * self.A),
                                                       _vp(self.sym_stat), stream), "lgx_ppo_mirror_loss_reduce")

    def resolve(self):
        """Apply a deferred update's readback (learning rate, losses); returns its losses, or None
        when nothing is pending."""
        n, self._pending = self._pending, None
        if n is None:
            return None
        self._pin_ev.synchronize()
        return self._apply_readback(self._pin_stats.tolist(), float(self._pin_lr[0]), n,
                                    float(self._pin_sym[0]) if self.ppo.mirror_loss_coeff is not None else None)

    def _gather_all(self, indices, obs, cobs, rows, stream):
        """The padded layer-1 input rows of the whole update in minibatch order: per minibatch the
        `xs` of _minibatch_body."""
        M = self.M
        # one input for both networks and dW1 on the library bmm: rows gathered twice per minibatch
        # ([nmb, 2, M, Kp]), so the layer-1 weight gradients of actor and critic are ONE batched GEMM
        if (cobs is None and self.num_obs == self.num_cobs and self.Xcp is None and 0 not in self.gemm_dw
                and self.run.dw1_batched):
            if self.Xall2 is None or self.Xall2.shape[0] * M != rows:
                self.Xall2 = torch.zeros(rows // M, 2, M, self.Kp, device=self.dev)
            self.check(self.lib.lgx_ppo_gather_rows_padded_dup(_vp(obs), _vp(self.Xall2), _vp(indices), rows,
                                                               obs.shape[1], self.Kp, M, stream), "gather")
            return [(x, None, x) for x in self.Xall2]
        if self.Xall is None or self.Xall.shape[0] != rows:
            self.Xall = torch.zeros(rows, self.Kp, device=self.dev)     # padding columns stay zero
            self.Xcall = torch.zeros(rows, self.Kcp, device=self.dev) if self.Xcp is not None else None
        self.check(self.lib.lgx_ppo_gather_rows_padded(_vp(obs), _vp(self.Xall), _vp(indices), rows, obs.shape[1],
                                                       self.Kp, stream), "gather")
        if cobs is not None:
            self.check(self.lib.lgx_ppo_gather_rows_padded(_vp(cobs), _vp(self.Xcall), _vp(indices), rows,
                                                           cobs.shape[1], self.Kcp, stream), "gather")
        return [tuple(x[i:i + M] if x is not None else None for x in (self.Xall, self.Xcall)) for i in range(0, rows, M)]

    def _loss_args(self, storage):
        a = abi.LgxPpoLossArgs()
        p = self.ppo
        a.rows, a.num_actions = self.M, self.A
        a.use_clipped_value_loss = int(bool(p.use_clipped_value_loss))
        a.clip_param, a.value_loss_coef, a.entropy_coef = p.clip_param, p.value_loss_coef, p.entropy_coef
        a.mu_raw, a.v_raw = self.MU.data_ptr(), self.V.data_ptr()
        a.b4a = self.flat_p.data_ptr() + 4 * self.bo[self.L]
        a.b4c = a.b4a + 4 * self.A
        a.std = self.flat_p.data_ptr() + 4 * self.std_off
        for k, v in storage.items():
            setattr(a, k, v.data_ptr())
        a.d_mu, a.d_v, a.partials = self.dMU.data_ptr(), self.dV.data_ptr(), self.loss_parts.data_ptr()
        a.g_b4a = self.flat_g.data_ptr() + 4 * self.bo[self.L]
        a.g_b4c = a.g_b4a + 4 * self.A
        a.g_std = self.flat_g.data_ptr() + 4 * self.std_off
        a.stats = self.stats.data_ptr()
        H = self.hidden[-1]
        if self.head_in_loss:   # (decided in _alloc)
            a.head_in, a.hidden = self.Y[self.L - 1].data_ptr(), H
            a.W4a, a.W4c = self.W[self.L][0].data_ptr(), self.W[self.L][1].data_ptr()
        else:
            a.head_in, a.W4a, a.W4c, a.hidden = None, None, None, 0
        a.defer_finalize = 1     # run by lgx_head_bwd_finalize / lgx_reduce_slices_finalize
        # single process with the adaptive schedule: the loss finalize adapts the learning rate
        # (data-parallel: lgx_ppo_adapt_lr after the all-reduce the KL rides in)
        if p.desired_kl is not None and p.schedule == "adaptive" and p.dist is None:
            a.lr, a.desired_kl = self.optimizer.lr_dev.data_ptr(), float(p.desired_kl)
        else:
            a.lr, a.desired_kl = None, 0.0
        self._keep = storage
        return a

    def gradients(self, idx, apply=False):
        """Flat gradient of one minibatch (rows `idx` of the current storage), for tests.  With the
        mirror loss: idx = rows, then the same rows' mirrors (rows + T x N)."""
        if self.recurrent:   # (a recurrent minibatch is whole envs through the memories: update())
            raise NotImplementedError("gradients(idx) takes feed-forward policies; recurrent ones go through update()")
        stream = self._begin_update(idx.numel(), reset=False)
        obs, cobs, storage = self._storage_views()
        self._minibatch(idx, obs, cobs, self._loss_args(storage), stream, apply=apply)
        if self.ppo.mirror_loss_coeff is not None:   # (sym_stat: this minibatch's L_sym)
            self._reduce_symmetry_loss(1)
        return self.flat_g.clone()

    # ------------------------------------------------------------------ GEMM timing (bench.py)
    def time_gemms(self, period):
        """Bracket every lgx_gemm_nt launch of every `period`-th minibatch with HIP events on the
        launch stream (0: off); gemm_timings() reads them back per epilogue (kernel instantiation).
        The data-parallel gradient all-reduces of those minibatches are bracketed too
        (comm_timings())."""
        self._t_period, self._t_count, self._t_events, self._t_mb = int(period), 0, [], 0
        self._c_events = []

    def _bracket(self, torch_stream=None):
        """In a timed minibatch (time_gemms): a pair of timing events, the first recorded on
        `torch_stream` (None: the current stream); the caller records the second.  Else None."""
        if not (self._t_period and self._t_count % self._t_period == 0):
            return None
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record(torch_stream)
        return ev

    def _all_reduce(self, buf, torch_stream):
        """ppo.dist.all_reduce(buf) issued on `torch_stream` (the current stream), with HIP events
        around it on that stream when this minibatch is timed."""
        ev = self._bracket(torch_stream)
        comm = self._lgx_comm()
        if comm is not None:   # lgx_allreduce_grads: RCCL on this stream itself (sum; 1/world in Adam)
            assert buf.dtype == torch.float32 and buf.is_contiguous()
            # one communicator, collectives issued from two streams (the bucketed update: side, then
            # main): RCCL orders nothing across streams, so a collective issued from another stream
            # than the previous one waits for it (torch's process group serialises on its own stream)
            prev = self._comm_last
            if prev is not None and prev[0] != torch_stream.cuda_stream:
                torch_stream.wait_event(prev[1])
            self.check(self.lib.lgx_allreduce_grads(comm, _vp(buf), buf.numel(), 0,
                                                    C.c_void_p(torch_stream.cuda_stream)), "allreduce_grads")
            done = torch.cuda.Event()
            done.record(torch_stream)
            self._comm_last = (torch_stream.cuda_stream, done)
        else:
            self.ppo.dist.all_reduce(buf)
        if ev:
            ev[1].record(torch_stream)
            self._c_events.append((buf.numel() * buf.element_size(), *ev))

    @property
    def allreduce_impl(self):
        """"lgx" (lgx_allreduce_grads on the library's own RCCL communicator, LGX_NATIVE_ALLREDUCE=1
        with the nccl backend) or "torch" (torch.distributed.all_reduce, the default)."""
        return "lgx" if self._comm not in (None, _UNTRIED) else "torch"

    def _lgx_comm(self):
        """The rank's lgx_comm, created collectively at the first gradient all-reduce when
        LGX_NATIVE_ALLREDUCE=1 and the process group is nccl (RCCL): rank 0 draws the unique id,
        the group broadcasts it; the RCCL library is torch's own (one RCCL instance per process)."""
        if self._comm is not _UNTRIED:
            return self._comm
        self._comm = None   # (tried: the torch path unless a communicator is created below)
        dist = self.ppo.dist
        if not _switches().native_allreduce:
            return None
        # asked for: fail loudly rather than fall back to torch.distributed (the 8-GPU run must use
        # the path it was configured for) or load an RCCL other than the one torch's nccl backend runs
        if dist.get_backend() != "nccl":
            raise RuntimeError(f"LGX_NATIVE_ALLREDUCE=1 needs the nccl (RCCL) process group, got {dist.get_backend()!r}")
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if not os.path.exists(path):
            raise RuntimeError(f"LGX_NATIVE_ALLREDUCE=1: torch's RCCL ({path}) is missing; refusing to load another "
                               "RCCL instance into the process")
        path = path.encode()
        uid = torch.zeros(abi.COMM_ID_BYTES, dtype=torch.uint8)
        if dist.get_rank() == 0:
            self.check(self.lib.lgx_comm_unique_id(path, C.cast(uid.data_ptr(), C.POINTER(C.c_uint8))),
                       "comm_unique_id")
        dev_uid = uid.to(self.dev)
        dist.broadcast(dev_uid, src=0)
        uid = dev_uid.cpu()
        comm = C.c_void_p()
        self.check(self.lib.lgx_comm_create(path, C.cast(uid.data_ptr(), C.POINTER(C.c_uint8)), dist.get_world_size(),
                                            dist.get_rank(), self.dev.index or 0, C.byref(comm)), "comm_create")
        self._comm = comm
        return comm

    def close_comm(self):
        """Destroy the lgx_comm (collective: every rank calls it after its last update)."""
        comm, self._comm = self._comm, None
        if comm not in (None, _UNTRIED):
            torch.cuda.synchronize(self.dev)
            self.check(self.lib.lgx_comm_destroy(comm), "comm_destroy")

    def comm_timings(self):
        """(collectives timed, total ms, total bytes, timed minibatches) of the all-reduces of the
        timed minibatches."""
        torch.cuda.synchronize()
        ev = self._c_events
        return len(ev), sum(e0.elapsed_time(e1) for _, e0, e1 in ev), sum(b for b, _, _ in ev), self._t_mb

    def _gemm(self, g, stream):
        ev = self._bracket()
        self.check(self.lib.lgx_gemm_nt(C.byref(g), stream), "gemm_nt")
        if ev:
            ev[1].record()
            # algorithmic FLOP: the unpadded K of layer 1 (num_obs), not the zero-padded columns
            k = self.k_alg.get(id(g), g.K)
            self._t_events.append((g.epi, 2.0 * g.M * g.N * k * g.batch, *ev))

    @property
    def join_events(self):
        """"device" (lgx_event_*) or "system" (torch events): the event kind an update started now
        would join its streams with (an update in progress keeps what it started with)."""
        return "device" if _switches().dev_events and self.ppo.dist is None else "system"

    def _side_stream(self):
        """The backward's second stream (with the torch events of its joins), created on first use."""
        if self._side is None:
            self._side = torch.cuda.Stream(self.dev)
            self._ev_in = [torch.cuda.Event() for _ in range(self.L)]
            self._ev_out = torch.cuda.Event()
        return self._side

    def _device_events(self):
        if self._dev_ev is None:
            self._dev_ev = []
            for _ in range(self.L + 1):
                e = C.c_void_p()
                self.check(self.lib.lgx_event_create(C.byref(e)), "event_create")
                self._dev_ev.append(e)
        return self._dev_ev

    def _arm(self, slot):
        """Bind join `slot`'s device event to the next lgx launch (the producer's last one), so the
        join records no separate event packet on the producer stream.  LGX_PPO_BIND=0, or torch
        events: recorded at the join."""
        if not self.run.bind:
            return
        self.check(self.lib.lgx_launch_bind_event(self._device_events()[slot]), "launch_bind_event")
        self._armed = slot

    def _join(self, src, dst, slot):
        """Order `dst` after the work issued so far on `src` (slot: 0..L-1 the side stream's inputs,
        L its output).  Device-scope events (lgx_event_*: no system-scope cache write-back and
        invalidate at the record) in single-process runs unless LGX_PPO_DEV_EVENTS=0 (torch
        events).  Data-parallel runs keep the system-scope events: the joins there also order the
        collectives' buffers, which peers write over xGMI."""
        if self.run.device_events:
            e = self._device_events()[slot]
            armed, self._armed = self._armed, None
            # bound to the producer's last launch by _arm (no record packet on `src`), else recorded
            if armed != slot or self.lib.lgx_launch_bind_pending():
                if armed is not None:
                    self.lib.lgx_launch_bind_pending()   # (a stale binding: disarm)
                self.check(self.lib.lgx_event_record(e, C.c_void_p(src.cuda_stream)), "event_record")
            self.check(self.lib.lgx_stream_wait_event(C.c_void_p(dst.cuda_stream), e), "stream_wait_event")
        else:
            e = self._ev_in[slot] if slot < self.L else self._ev_out
            e.record(src)
            dst.wait_event(e)

    def __del__(self):
        for e in self._dev_ev or []:
            try:
                self.lib.lgx_event_destroy(e)
            except Exception:
                pass

    def _gemm_tn(self, t, stream, torch_stream=None):
        ev = self._bracket(torch_stream)   # (events on the stream the kernel runs on)
        self.check(self.lib.lgx_gemm_tn(C.byref(t), stream), "gemm_tn")
        if ev:
            ev[1].record(torch_stream)
            self._t_events.append(("tn", 2.0 * t.M * t.R * t.Cc * t.batch, *ev))

    def gemm_timings(self):
        """{epilogue: (launches, total ms, total algorithmic FLOP, timed minibatches)} of the timed
        launches."""
        torch.cuda.synchronize()
        out = {}
        for epi, flop, e0, e1 in self._t_events:
            n, ms, f, _ = out.get(epi, (0, 0.0, 0.0, 0))
            out[epi] = (n + 1, ms + e0.elapsed_time(e1), f + flop, self._t_mb)
        return out

    # ------------------------------------------------------------------ one minibatch
    @torch.no_grad()
    def _minibatch(self, idx, obs, cobs, args, stream, apply=True, xs=None):
        with self.tuned:     # TunableOp table on for the library GEMMs of this minibatch only
            self._minibatch_body(idx, obs, cobs, args, stream, apply, xs)

    def _minibatch_body(self, idx, obs, cobs, args, stream, apply=True, xs=None):
        """One minibatch: rows `idx` of the storage; `xs` = their padded layer-1 inputs already
        gathered (slices of _gather_all's buffers), None = gather here.  `stream` is the current
        stream's handle; the run switches are those of the enclosing update() / gradients() call."""
        ppo = self.ppo
        if self._t_period:
            self._t_mb += self._t_count % self._t_period == 0
            self._t_count += 1
        if self.lgx_gemm:
            inp = self._inputs_lgx(idx, obs, cobs, stream, xs)
            self._forward_lgx(stream)
        else:
            inp = self._inputs_lib(idx, obs, cobs, stream)
            self._forward_lib(inp, stream)
        self._loss_and_heads(idx, args, stream)
        dZ, side_used = self._backward_lgx(stream) if self.lgx_gemm else self._backward_lib(stream)
        # every gradient block but dW1's is complete once dA_1 (this stream) and the side stream's
        # dW GEMMs are: they are reduced early, on the side stream, while dW1 runs here
        early = side_used and self.loss_bwd and len(self.jobs_rest) > 0 and self.run.early_reduce
        # the clip norm's sums of squares from the reduction launches (their buffer, or 0)
        sq = self.sq_parts.data_ptr() if self.fused_sq and apply and ppo.dist is None else 0
        self.bucketed = early and apply and ppo.dist is not None and not self.recurrent
        if early:
            self._reduce_rest_on_side(args, sq)
        self._dw1(inp, dZ, stream)
        nsq = self._reduce(args, sq, early, side_used, stream)
        if self.recurrent:
            self._memory_backward()
        if apply:
            grad_scale = self._all_reduce_gradient(stream) if ppo.dist is not None else 1.0
            self._optimizer_step(sq, nsq, grad_scale, stream)

    # ---- inputs: the layer-1 rows of both networks.  X / Xc are the unpadded rows (library
    # GEMMs), xp / xcp the rows padded to the GEMM's K step (lgx GEMMs; xcp None: one input for
    # both networks), dup the [2, M, Kp] block of _gather_all's duplicated rows (batched dW1)
    def _inputs_lgx(self, idx, obs, cobs, stream, xs):
        lib, chk, M = self.lib, self.check, self.M
        if not self._mirrors_valid:   # (afterwards lgx_adam_clip_mirror keeps the weight copies current)
            if self.split:
                chk(lib.lgx_split_bf16(self.copy_jobs, len(self.copy_jobs), stream), "split_bf16")
            else:
                chk(lib.lgx_copy2d(self.copy_jobs, len(self.copy_jobs), stream), "copy2d")
            self._mirrors_valid = True
        dup = None
        if xs is None:
            chk(lib.lgx_ppo_gather_rows_padded(_vp(obs), _vp(self.Xp), _vp(idx), M, obs.shape[1], self.Kp,
                                               stream), "gather")
            if cobs is not None:
                chk(lib.lgx_ppo_gather_rows_padded(_vp(cobs), _vp(self.Xcp), _vp(idx), M, cobs.shape[1],
                                                   self.Kcp, stream), "gather")
            xp, xcp = self.Xp, self.Xcp
        elif len(xs) > 2:                   # [2, M, Kp]: net 0's copy feeds the forward
            xp, xcp, dup = xs[0][0], xs[1], xs[2]
        else:
            xp, xcp = xs
        X = Xc = xp[:, :self.num_obs]
        if cobs is not None or self.recurrent:
            Xc = xcp[:, :self.num_cobs]
        for g, x in zip(self.gemm_fwd[0], (xp, xcp if xcp is not None else xp)):   # (one launch, or one per network)
            g.A = x.data_ptr()
        return SimpleNamespace(X=X, Xc=Xc, xp=xp, xcp=xcp, dup=dup)

    def _inputs_lib(self, idx, obs, cobs, stream):
        lib, chk, M = self.lib, self.check, self.M
        X = Xc = self.X
        chk(lib.lgx_ppo_gather_rows(_vp(obs), _vp(X), _vp(idx), M, obs.shape[1], stream), "gather")
        if cobs is not None:
            Xc = self.Xc
            chk(lib.lgx_ppo_gather_rows(_vp(cobs), _vp(Xc), _vp(idx), M, cobs.shape[1], stream), "gather")
        return SimpleNamespace(X=X, Xc=Xc, xp=None, xcp=None, dup=None)

    # ---- forward: the hidden layers into Y[k] ([2, M, h_k], actor and critic batched)
    def _forward_lgx(self, stream):
        for g in self.gemm_fwd[0]:
            self._gemm(g, stream)
        for k in range(1, self.L):
            if k in self.lgx_fwd_layers:
                self._gemm(self.gemm_fwd[k], stream)
            else:                           # (LGX_PPO_GEMM=auto)
                self._bmm_bias_elu(k, stream)

    def _forward_lib(self, inp, stream):
        if inp.Xc is inp.X:   # shared input: one batched GEMM over {actor, critic} with a stride-0 input
            torch.bmm(inp.X.unsqueeze(0).expand(2, self.M, self.num_obs), self.W1s.transpose(1, 2), out=self.Y[0])
        else:
            wa, wc = self.W[0]
            torch.mm(inp.X, wa.t(), out=self.Y[0][0])
            torch.mm(inp.Xc, wc.t(), out=self.Y[0][1])
        self._bias_elu(0, stream)
        for k in range(1, self.L):
            self._bmm_bias_elu(k, stream)

    def _bmm_bias_elu(self, k, stream):
        """Hidden layer k >= 1 on the library GEMM + lgx_bias_act."""
        torch.bmm(self.Y[k - 1], self.W[k].transpose(1, 2), out=self.Y[k])
        self._bias_elu(k, stream)

    def _bias_elu(self, k, stream):
        self.check(self.lib.lgx_bias_act(_vp(self.Y[k]), C.c_void_p(self.flat_p.data_ptr() + 4 * self.bo[k]), self.M,
                                         self.hidden[k], 2, 1, stream), "bias")

    # ---- loss, gradient at the heads (dZ of the last hidden layer, in place over Y[L-1]), KL ->
    # adaptive learning rate (single process: in the loss finalize)
    def _loss_and_heads(self, idx, args, stream):
        lib, chk, L = self.lib, self.check, self.L
        wha, whc = self.W[L]
        if not self.head_in_loss:
            torch.mm(self.Y[L - 1][0], wha.t(), out=self.MU)
            torch.mm(self.Y[L - 1][1], whc.t(), out=self.V)
        args.idx = idx.data_ptr()
        if self.loss_bwd:
            # loss + output-layer backward in one launch; its finalize runs in the reduction
            if self.run.side_on and (L - 1) in self.gemm_dw:
                self._arm(L - 1)   # (the first join's producer)
            if self.ppo.mirror_loss_coeff is not None:   # (the plan runs this launch: checked in _alloc)
                chk(lib.lgx_ppo_loss_bwd_mirror(C.byref(args), *self._mirror_args(), _vp(self.head_parts), stream),
                    "lgx_ppo_loss_bwd_mirror")
            else:
                chk(lib.lgx_ppo_loss_bwd(C.byref(args), _vp(self.head_parts), stream), "lgx_ppo_loss_bwd")
        else:
            chk(lib.lgx_ppo_loss(C.byref(args), stream), "lgx_ppo_loss")
            # output-layer backward (+ the loss finalize on one extra workgroup of the same launch)
            chk(lib.lgx_head_bwd_finalize(C.byref(args), _vp(self.dMU), _vp(self.dV), _vp(wha), _vp(whc),
                                          _vp(self.Y[L - 1]), self.M, self.A, self.hidden[-1], _vp(self.head_parts),
                                          stream), "head_bwd")

    # ---- backward through the hidden layers L-1 .. 1: dW_k = dZ_k^T Y_{k-1} split-K over Sk[k] row
    # slices into P[k] (reduced later), dZ_{k-1} = (dZ_k W_k) * elu'(Y_{k-1}), dZ_{L-1} in Y[L-1].
    # Both return (dZ_1, whether the side stream was used)
    def _backward_lgx(self, stream):
        """dW_k (lgx_gemm_tn) on a second stream, each right after its own join, concurrent with
        dA_k on this one (both only read dZ_k and Y_{k-1}); LGX_PPO_DW_SIDE=0 keeps every launch
        on one stream; a dW that is not on lgx_gemm_tn takes the library bmm on this one."""
        L, dw = self.L, self.gemm_dw
        side = main = None
        if self.run.side_on and any(k in dw for k in range(1, L)):
            side, main = self._side_stream(), torch.cuda.current_stream(self.dev)
        dw_stream = C.c_void_p(side.cuda_stream) if side is not None else stream
        for k in range(L - 1, 0, -1):
            if k not in dw:
                self._dw_bmm(k)
            else:
                if side is not None:
                    self._join(main, side, k)
                for t in dw[k]:
                    self._gemm_tn(t, dw_stream, side)
            if side is not None and k - 1 >= 1 and (k - 1) in dw:
                self._arm(k - 1)   # (the next join's producer: this dA launch)
            self._gemm(self.gemm_bwd[k], stream)
        return self._dz(0), side is not None

    def _backward_lib(self, stream):
        for k in range(self.L - 1, 0, -1):
            self._dw_bmm(k)
            torch.bmm(self._dz(k), self.W[k], out=self.D[k - 1])
            self.check(self.lib.lgx_elu_bwd_colsum(_vp(self.D[k - 1]), _vp(self.Y[k - 1]), self.M, self.hidden[k - 1], 2,
                                                   _vp(self.col_parts[k - 1]), stream), "elu_bwd")
        return self._dz(0), False

    def _dz(self, k):
        return self.Y[k] if k == self.L - 1 else self.D[k]

    def _dw_bmm(self, k):
        """dW_k, k >= 1, on the library bmm over the row slices."""
        M, Sl, h = self.M, self.Sk[k], self.hidden
        torch.bmm(self._dz(k).view(2 * Sl, M // Sl, h[k]).transpose(1, 2),
                  self.Y[k - 1].view(2 * Sl, M // Sl, h[k - 1]), out=self.P[k])

    def _dw1(self, inp, dZ, stream):
        """The layer-1 weight gradient, on the main stream."""
        M, S, h = self.M, self.S, self.hidden
        if 0 in self.gemm_dw:               # lgx_gemm_tn over the minibatch's padded input rows
            for t, x in zip(self.gemm_dw[0], (inp.xp, inp.xcp if inp.xcp is not None else inp.xp)):
                t.B = x.data_ptr()
                self._gemm_tn(t, stream)
        elif inp.dup is not None:           # one batched GEMM: 2 networks x S row slices
            x2 = inp.dup.view(2 * S, M // S, self.Kp)[:, :, :self.num_obs]
            torch.bmm(dZ.view(2 * S, M // S, h[0]).transpose(1, 2), x2, out=self.P[0].view(2 * S, h[0], self.num_obs))
        else:
            torch.bmm(dZ[0].view(S, M // S, h[0]).transpose(1, 2), inp.X.unflatten(0, (S, M // S)), out=self.P[0][0])
            torch.bmm(dZ[1].view(S, M // S, h[0]).transpose(1, 2), inp.Xc.unflatten(0, (S, M // S)), out=self.P[0][1])

    # ---- reductions of the split-K / bias partials into the flat gradient; data-parallel buckets
    def _reduce_launch(self, jobs, args, sq, stream):
        """One reduction launch over `jobs`; args: with the loss finalize (loss_bwd); sq: writing the
        clip norm's sum-of-squares partials there (the step counter advanced with the finalize)."""
        lib, n = self.lib, len(jobs)
        if sq:
            rc = lib.lgx_reduce_slices_sq(jobs, n, C.byref(args) if args is not None else None, C.c_void_p(sq),
                                          _vp(self.optimizer.step_dev) if args is not None else None, stream)
        elif args is not None:
            rc = lib.lgx_reduce_slices_finalize(jobs, n, C.byref(args), stream)
        else:
            rc = lib.lgx_reduce_slices(jobs, n, stream)
        self.check(rc, "reduce")

    def _reduce_rest_on_side(self, args, sq):
        """The early reduction: every job but dW1's (+ the loss finalize) on the side stream, the
        memory-bound reduction next to the MFMA-bound dW1 GEMM on the main one.  Data-parallel:
        that bucket (every block after dW1's in the flat layout + the KL slot) is all-reduced from
        the side stream right away; dW1's follows in _reduce (one communicator: the collectives run
        in issue order on every rank)."""
        side = self._side
        if not self.rest_on_side:   # (a rest job reads a dA epilogue's partials from the main stream)
            self._join(torch.cuda.current_stream(self.dev), side, 0)
        self._arm(self.L)   # (the final join's producer: the side stream's last launch)
        self._reduce_launch(self.jobs_rest, args, sq, C.c_void_p(side.cuda_stream))
        if self.bucketed:
            with torch.cuda.stream(side):
                self.g_comm[self.n:].copy_(self.stats[0:1])
                self._all_reduce(self.g_comm[self.nW1:], side)

    def _reduce(self, args, sq, early, side_used, stream):
        """On the main stream after dW1: its jobs (early: the rest is on the side stream, joined
        here) or all jobs in one launch.  Returns the number of sum-of-squares partials written."""
        main = torch.cuda.current_stream(self.dev)
        if not early:
            if side_used:   # the weight gradients are complete before the reduction reads them
                self._join(self._side, main, self.L)
            sq = sq if self.loss_bwd else 0
            self._reduce_launch(self.jobs, args if self.loss_bwd else None, sq, stream)
            return self.nsq_all if sq else 0
        self._reduce_launch(self.jobs_dw1, None, sq + 4 * self.nsq_rest if sq else 0, stream)
        if self.bucketed:
            self._all_reduce(self.g_comm[:self.nW1], main)
        self._join(self._side, main, self.L)
        return self.nsq_rest + self.nsq_dw1 if sq else 0

    def _all_reduce_gradient(self, stream):
        """Data-parallel: summed gradient + summed KL (rsl_rl adapts the LR before the step, only
        the optimizer step reads it, so adapting after the backward is equivalent): the two buckets
        issued by the reductions, or one collective here.  Returns the gradient's scale 1 / world."""
        ppo = self.ppo
        if not self.bucketed:
            self.g_comm[self.n:].copy_(self.stats[0:1])
            self._all_reduce(self.g_comm, torch.cuda.current_stream(self.dev))
        grad_scale = 1.0 / ppo.dist.get_world_size()
        if ppo.desired_kl is not None and ppo.schedule == "adaptive":
            self.check(self.lib.lgx_ppo_adapt_lr(C.c_void_p(self.g_comm.data_ptr() + 4 * self.n), grad_scale,
                                                 _vp(self.optimizer.lr_dev), ppo.desired_kl, stream), "adapt_lr")
        return grad_scale

    # ---- optimizer step: clip_grad_norm_ + Adam on the flat buffers
    def _optimizer_step(self, sq, nsq, grad_scale, stream):
        lib, o, clip = self.lib, self.optimizer, self.ppo.max_grad_norm
        bufs = (_vp(self.flat_p), _vp(self.flat_g), _vp(o.m), _vp(o.v), self.n)
        norm = (_vp(self.norm_parts), self.norm_parts.numel(), grad_scale, clip)   # (its own sum-of-squares pass)
        adam = (_vp(o.lr_dev), _vp(o.step_dev), o.betas[0], o.betas[1], o.eps)
        mirrors = (self.copy_jobs, len(self.copy_jobs)) if self.lgx_gemm else ()   # the GEMM weight copies, kept current
        if mirrors and nsq:   # (norm from the reductions' sums of squares; step advanced there)
            rc = lib.lgx_adam_clip_mirror_sq(*bufs, C.c_void_p(sq), nsq, clip, *adam, *mirrors, stream)
        elif mirrors:
            rc = lib.lgx_adam_clip_mirror(*bufs, *norm, *adam, *mirrors, stream)
        else:
            rc = lib.lgx_adam_clip(*bufs, *norm, *adam, stream)
        self.check(rc, "adam")

