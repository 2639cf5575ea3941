"""Empirical observation normalisation (rsl_rl 2.x `EmpiricalNormalization`): a running mean and
population standard deviation per observation column, updated during collection and applied in
front of the policy and the critic.

The state is float64: `n`, `mean[D]`, `m2[D]` (sum of squared deviations), all zeros when empty.
A training call on a batch `x [N, D]` (float32)

1. cuts the rows into consecutive blocks of `R = rows_per_part()` rows (the last may be shorter)
   and computes each block's float64 `(n_b, mean_b, m2_b)` per column, rows in ascending order;
2. folds the blocks into the state in ascending order with Chan's combine
   (`n = n_a + n_b, d = mean_b - mean_a, w = n_b / n, mean = mean_a + d w, m2 = m2_a + m2_b + d^2 n_a w`);
   data-parallel runs (world > 1 or LGX_DIST_REHEARSAL=1) all-gather every rank's blocks first and
   fold them all, ranks in order, so every rank holds the same state;
3. returns `y = (x - float(mean)) * float(1 / (sqrt(m2 / n) + eps))`: the statistics include the
   current batch (update first, then normalise, as rsl_rl does).

A frozen call does step 3 only (an empty normaliser: mean 0, std 1).  A training call once
`n >= until` is a frozen call.  The order of every sum is fixed, so two runs agree bitwise, and
W ranks x N / W envs agree bitwise with one process x N envs when N / W is a multiple of R.

On a CUDA device steps 1 and 2 + 3 are one launch each of csrc/lgx_obsnorm.hip, for up to two
normalisers together (`normalize_many`), with no fallback; on the CPU the same partition and fold
order in torch float64.
"""
import ctypes as C

import torch

from legged_gym_amd.sim import abi


def rows_per_part():
    """R: rows per partial summary, a constant of the library (LGX_OBS_NORM_ROWS)."""
    return abi.OBS_NORM_ROWS


def _dist():
    from .ppo import _dist as ppo_dist
    return ppo_dist()


def _gather(parts):
    """Every rank's partials, concatenated in rank order (the pattern of PPO._gather_moments)."""
    dist = _dist()
    if dist is None:
        return parts
    out = [torch.empty_like(parts) for _ in range(dist.get_world_size())]
    dist.all_gather(out, parts.contiguous())
    return torch.cat(out)


def partials_torch(x):
    """[P, 1 + 2 D] float64 block summaries of x [N, D], in the library's layout and order."""
    R = rows_per_part()
    x = x.detach().to(torch.float64)
    N, D = x.shape
    out = []
    for blocks in (x[:N - N % R].view(-1, R, D), x[N - N % R:].view(1, -1, D)):
        nb, nr = blocks.shape[0], blocks.shape[1]
        if nb == 0 or nr == 0:
            continue
        s = torch.zeros(nb, D, dtype=torch.float64)
        for i in range(nr):          # ascending rows: the order is part of the result
            s = s + blocks[:, i]
        mean = s / nr
        m2 = torch.zeros(nb, D, dtype=torch.float64)
        for i in range(nr):
            d = blocks[:, i] - mean
            m2 = m2 + d * d
        out.append(torch.cat([torch.full((nb, 1), float(nr), dtype=torch.float64), mean, m2], dim=1))
    return torch.cat(out)


def merge_torch(state, parts):
    """The state [1 + 2 D] after folding parts [P, 1 + 2 D] into it in ascending order."""
    D = (state.numel() - 1) // 2
    n, mean, m2 = float(state[0]), state[1:1 + D].clone(), state[1 + D:].clone()
    for p in parts:
        nb = float(p[0])
        tot = n + nb
        if tot == 0.0:
            continue
        w = nb / tot
        d = p[1:1 + D] - mean
        mean = mean + d * w
        m2 = (m2 + p[1 + D:]) + d * d * (n * w)
        n = tot
    return torch.cat([torch.tensor([n], dtype=torch.float64), mean, m2])


def apply_torch(state, x, eps):
    D = x.shape[1]
    n = float(state[0])
    if n > 0:
        mean, std = state[1:1 + D], torch.sqrt(state[1 + D:] / n)
    else:
        mean, std = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    return (x - mean.to(torch.float32)) * (1.0 / (std + eps)).to(torch.float32)


class EmpiricalNormalization:
    def __init__(self, width, eps=1e-2, until=None, device="cpu"):
        self.width, self.eps, self.until = int(width), float(eps), until
        if not 1 <= self.width <= abi.MAX_PRIV_OBS:
            raise ValueError(f"EmpiricalNormalization: width must be in 1..{abi.MAX_PRIV_OBS}")
        self.device = torch.device(device)
        self.on_device = self.device.type == "cuda"
        self._count = 0        # the state's n, kept on the host as well: `until` costs no readback
        # a training launch reads _states[_cur] and writes the other one
        self._states = [torch.zeros(1 + 2 * self.width, dtype=torch.float64, device=self.device) for _ in range(2)]
        self._cur = 0
        self._out = [None, None]   # the result stays valid until the call after next
        self._next = 0
        self._parts = None
        self._lib = None
        if self.on_device:
            from legged_gym_amd.sim import lib as lgx_lib
            self._lib, self._check = lgx_lib.load(), lgx_lib.check
            if self._lib.lgx_obs_norm_rows_per_part() != abi.OBS_NORM_ROWS:
                raise lgx_lib.LgxError("liblgx.so: LGX_OBS_NORM_ROWS differs from abi.OBS_NORM_ROWS")

    # ------------------------------------------------------------------ state
    @property
    def _state(self):
        return self._states[self._cur]

    @property
    def count(self):
        if self._count is None:   # after apply() with the caller's partials: n is only on the device
            self._count = int(self._state[0].item())
        return self._count

    @property
    def mean(self):
        return self._state[1:1 + self.width].to(torch.float32)

    @property
    def std(self):
        if self.count == 0:
            return torch.ones(self.width, dtype=torch.float32, device=self.device)
        return torch.sqrt(self._state[1 + self.width:] / self.count).to(torch.float32)

    def inv(self):
        """float32 1 / (std + eps), the factor a frozen call multiplies by."""
        if self.count == 0:
            std = torch.ones(self.width, dtype=torch.float64, device=self.device)
        else:
            std = torch.sqrt(self._state[1 + self.width:] / self.count)
        return (1.0 / (std + self.eps)).to(torch.float32)

    def state_dict(self):
        s = self._state.detach().cpu()
        return {"count": torch.tensor(int(s[0]), dtype=torch.int64), "mean": s[1:1 + self.width].clone(),
                "m2": s[1 + self.width:].clone()}

    def load_state_dict(self, d):
        mean, m2 = d["mean"].to(torch.float64).reshape(-1), d["m2"].to(torch.float64).reshape(-1)
        if mean.numel() != self.width or m2.numel() != self.width:
            raise ValueError(f"EmpiricalNormalization: state of width {mean.numel()} loaded into width {self.width}")
        self._count = int(d["count"])
        s = torch.cat([torch.tensor([float(self._count)], dtype=torch.float64), mean.cpu(), m2.cpu()])
        self._states[self._cur] = s.to(self.device)

    def to(self, device):
        """This normaliser with its state on `device` (itself when already there)."""
        device = torch.device(device)
        if device.type == self.device.type and (device.index == self.device.index or
                                                None in (device.index, self.device.index)):
            return self
        other = EmpiricalNormalization(self.width, self.eps, self.until, device)
        other.load_state_dict(self.state_dict())
        return other

    def frozen(self):
        return self.until is not None and self.count >= self.until

    # ------------------------------------------------------------------ calls
    def __call__(self, x, update=None):
        """The normalised x; update=None: a training call (frozen once count >= until)."""
        return normalize_many([self], [x], update)[0]

    def partials(self, x):
        """This rank's block summaries of x, [P, 1 + 2 width] float64 (step 1 alone)."""
        return _partials([self], [self._check_input(x)])[0].clone()

    def apply(self, x, parts=None):
        """Step 2 + 3 with the given partials (None: step 3 alone, a frozen call)."""
        x = self._check_input(x)
        return _apply([self], [x], [parts], [parts is not None])[0]

    def _check_input(self, x):
        if x.dim() != 2 or x.shape[1] != self.width or x.shape[0] < 1 or x.dtype != torch.float32:
            raise ValueError(f"EmpiricalNormalization: expected float32 [N >= 1, {self.width}], got "
                             f"{x.dtype} {tuple(x.shape)}")
        if x.device.type != self.device.type:
            raise ValueError(f"EmpiricalNormalization on {self.device} called with a tensor on {x.device}")
        return x.contiguous()

    def _out_buf(self, x):
        slot = self._next
        self._next ^= 1
        if self._out[slot] is None or self._out[slot].shape != x.shape:
            self._out[slot] = torch.empty_like(x)
        return self._out[slot]

    def _parts_buf(self, rows):
        P = -(-rows // rows_per_part())
        if self._parts is None or self._parts.shape[0] != P:
            self._parts = torch.empty(P, 1 + 2 * self.width, dtype=torch.float64, device=self.device)
        return self._parts


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _partials(norms, xs):
    if not norms[0].on_device:
        return [partials_torch(x) for x in xs]
    jobs = (abi.LgxObsNormJob * len(norms))()
    parts = [nz._parts_buf(x.shape[0]) for nz, x in zip(norms, xs)]
    for j, nz, x, p in zip(jobs, norms, xs, parts):
        j.x, j.rows, j.width, j.parts = x.data_ptr(), x.shape[0], nz.width, p.data_ptr()
    lib = norms[0]._lib
    norms[0]._check(lib.lgx_obs_norm_partials(jobs, len(norms), _stream(xs[0].device)), "lgx_obs_norm_partials")
    return parts


def _apply(norms, xs, parts, updates):
    """Step 2 (where updates[i]) + step 3 for each normaliser, one launch on the device."""
    if not norms[0].on_device:
        ys = []
        for nz, x, p, up in zip(norms, xs, parts, updates):
            if up:
                nz._states[nz._cur ^ 1] = merge_torch(nz._state, p)
                nz._cur ^= 1
                nz._count = int(nz._state[0])
            ys.append(apply_torch(nz._state, x, nz.eps))
        return ys
    jobs = (abi.LgxObsNormJob * len(norms))()
    ys = [nz._out_buf(x) for nz, x in zip(norms, xs)]
    for j, nz, x, y, p, up in zip(jobs, norms, xs, ys, parts, updates):
        j.x, j.y, j.rows, j.width, j.update, j.eps = x.data_ptr(), y.data_ptr(), x.shape[0], nz.width, int(up), nz.eps
        j.state_in = nz._state.data_ptr()
        if up:
            p = p.contiguous()
            j.parts, j.nparts, j.state_out = p.data_ptr(), p.shape[0], nz._states[nz._cur ^ 1].data_ptr()
    lib = norms[0]._lib
    norms[0]._check(lib.lgx_obs_norm_apply(jobs, len(norms), _stream(xs[0].device)), "lgx_obs_norm_apply")
    for nz, up in zip(norms, updates):
        if up:
            nz._cur ^= 1
            nz._count = None
    return ys


def normalize_many(norms, xs, update=None):
    """`[nz(x) for nz, x in zip(norms, xs)]` for up to two distinct normalisers on one device, in at
    most two launches for all of them together."""
    if not 1 <= len(norms) <= abi.OBS_NORM_MAX_JOBS or len(norms) != len(xs) or len({id(n) for n in norms}) != len(norms):
        raise ValueError(f"normalize_many: 1..{abi.OBS_NORM_MAX_JOBS} distinct normalisers, one tensor each")
    xs = [nz._check_input(x) for nz, x in zip(norms, xs)]
    ups = [(update is None or bool(update)) and not nz.frozen() for nz in norms]
    parts = [None] * len(norms)
    counts = [nz.count for nz in norms]
    training = [i for i, up in enumerate(ups) if up]
    if training:
        local = _partials([norms[i] for i in training], [xs[i] for i in training])
        for i, p in zip(training, local):
            parts[i] = _gather(p)
            counts[i] += xs[i].shape[0] * (parts[i].shape[0] // p.shape[0])   # (every rank: the same rows)
    ys = _apply(norms, xs, parts, ups)
    for nz, n in zip(norms, counts):
        nz._count = n   # known on the host: `until` and `count` cost no readback
    return ys
