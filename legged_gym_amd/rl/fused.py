"""Python shims over the PPO-side HIP kernels of liblgx.so (no fallback on GPU tensors)."""
import ctypes as C

import torch

from legged_gym_amd.sim import lib as lgxlib

_scratch = {}   # gae_norm's, by (device, envs)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def stream_of(t):
    """The current stream of t's device, as the library's entries take it."""
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _gae(entry, arrays, gamma, lam, *extra):
    """One lgx_gae* launch.  arrays = (rewards, values, dones, last_values, returns, advantages):
    rewards/values/returns/advantages [T,N,1] f32, dones [T,N,1] uint8, last_values [N,1];
    extra: the entry's trailing device buffers."""
    T, N = arrays[0].shape[0], arrays[0].shape[1]
    for t in arrays:
        assert t.is_cuda and t.is_contiguous()
    lgxlib.check(getattr(lgxlib.load(), entry)(*map(_vp, arrays), T, N, float(gamma), float(lam), *map(_vp, extra),
                                               stream_of(arrays[0])), entry)


def _norm_scratch(rewards):
    return torch.empty(int(lgxlib.load().lgx_gae_norm_scratch(rewards.shape[1])), dtype=torch.float64,
                       device=rewards.device)


def gae(rewards, values, dones, last_values, returns, advantages, gamma, lam):
    """rewards/values/returns/advantages [T,N,1] f32, dones [T,N,1] uint8, last_values [N,1]."""
    _gae("lgx_gae", (rewards, values, dones, last_values, returns, advantages), gamma, lam)


def gae_norm(rewards, values, dones, last_values, returns, advantages, gamma, lam):
    """gae() + rsl_rl's advantage normalisation in place (single process): lgx_gae_norm."""
    key = (rewards.device, rewards.shape[1])
    if key not in _scratch:
        _scratch[key] = _norm_scratch(rewards)
    _gae("lgx_gae_norm", (rewards, values, dones, last_values, returns, advantages), gamma, lam, _scratch[key])


def gae_parts(rewards, values, dones, last_values, returns, advantages, gamma, lam):
    """gae() + this rank's per-workgroup (count, mean, M2) advantage summaries (lgx_gae_parts):
    returns the [lgx_gae_norm_scratch(N)] float64 device tensor (data-parallel normalisation)."""
    parts = _norm_scratch(rewards)
    _gae("lgx_gae_parts", (rewards, values, dones, last_values, returns, advantages), gamma, lam, parts)
    return parts


def adv_norm(advantages, parts):
    """Normalise `advantages` in place with the statistics of the (count, mean, M2) summaries
    `parts` (every rank's, in rank order): lgx_adv_norm."""
    assert advantages.is_cuda and advantages.is_contiguous() and parts.is_cuda and parts.dtype == torch.float64
    parts = parts.contiguous()
    assert parts.numel() % 3 == 0
    lgxlib.check(lgxlib.load().lgx_adv_norm(_vp(advantages), advantages.numel(), _vp(parts), parts.numel() // 3,
                                            stream_of(advantages)), "lgx_adv_norm")
