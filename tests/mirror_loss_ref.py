"""Float64 statement of one PPO minibatch's loss with the symmetry mirror loss (rsl_rl 2.x
`PPO.update` with symmetry_cfg.use_mirror_loss), written from the formulas and not
through legged_gym_amd.rl.ppo: the reference of tests/test_mirror_loss.py (the unfused path) and
tests/test_gpu_mirror_loss.py (lgx_ppo_loss_bwd_mirror on its own).

A minibatch is M rollout rows followed by their M mirror images.  `ppo_rows` = 2 M: the PPO terms
run over all rows (with data augmentation); `ppo_rows` = M: over the rollout rows alone, the
mirror rows carry only the mirror term.  `coeff` None: no mirror term (plain PPO over ppo_rows rows).
"""
import math

import torch

F64 = torch.float64


def ppo_terms(mu, value, std, batch, clip=0.2, clipped_value=True):
    """(surrogate loss, value loss, entropy mean, KL mean) over the rows given, float64.
    mu [R, A], value [R], std [A]; batch: actions, old_mu, old_sigma [R, A]; old_logp, advantages,
    target_values, returns [R]."""
    var = std * std
    logp = (-(batch["actions"] - mu) ** 2 / (2 * var) - torch.log(std) - 0.5 * math.log(2 * math.pi)).sum(-1)
    ratio = torch.exp(logp - batch["old_logp"])
    adv = batch["advantages"]
    surrogate = torch.maximum(-adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)).mean()
    tv, ret = batch["target_values"], batch["returns"]
    if clipped_value:
        vc = tv + (value - tv).clamp(-clip, clip)
        value_loss = torch.maximum((value - ret) ** 2, (vc - ret) ** 2).mean()
    else:
        value_loss = ((ret - value) ** 2).mean()
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).sum()       # the same for every row
    so, mo = batch["old_sigma"], batch["old_mu"]
    kl = (torch.log(std / so + 1e-5) + (so * so + (mo - mu) ** 2) / (2 * var) - 0.5).sum(-1).mean()
    return surrogate, value_loss, entropy, kl


def symmetry_loss(mu, perm, sign):
    """L_sym = mean over M x A of (mu(o'_r)[j] - sign[j] mu(o_r)[perm[j]])^2; the target is detached."""
    M = mu.shape[0] // 2
    target = (mu[:M].detach()[:, perm.long()] * sign.to(mu.dtype))
    return ((mu[M:] - target) ** 2).mean()


def minibatch_loss(mu, value, std, batch, ppo_rows, coeff=None, perm=None, sign=None, clip=0.2, value_loss_coef=1.0,
                   entropy_coef=0.01, clipped_value=True):
    """-> dict(loss, surrogate, value_loss, kl, symmetry) in float64 (symmetry None without coeff)."""
    n = ppo_rows
    head = {k: v[:n] for k, v in batch.items()}
    s, vl, ent, kl = ppo_terms(mu[:n], value[:n], std, head, clip, clipped_value)
    loss = s + value_loss_coef * vl - entropy_coef * ent
    lsym = None
    if coeff is not None:
        lsym = symmetry_loss(mu, perm, sign)
        loss = loss + coeff * lsym
    return dict(loss=loss, surrogate=s, value_loss=vl, kl=kl, symmetry=lsym)


def to64(batch):
    return {k: v.detach().to(F64) for k, v in batch.items()}


def head_reference(A3, W4a, b4a, W4c, b4c, std, batch, ppo_rows, coeff, perm, sign, **kw):
    """What lgx_ppo_loss_bwd_mirror computes from the last hidden activations A3 [2, R, H] (post-ELU:
    actor, critic): autograd in float64 of minibatch_loss through the two output layers.
    -> dict: dZ3 [2, R, H] (= dL/dA3 * ELU'(z3), ELU' from the output: 1 for y > 0, else y + 1), dW4a,
    dW4c, db3 [2, H] (column sums of dZ3), g_std, g_b4a, g_b4c, kl, surrogate, value_loss, symmetry."""
    leaf = lambda x: x.detach().to(F64).clone().requires_grad_(True)
    A3, W4a, b4a, W4c, b4c, std = (leaf(x) for x in (A3, W4a, b4a, W4c, b4c, std))
    mu = A3[0] @ W4a.t() + b4a
    value = (A3[1] @ W4c.t()).squeeze(-1) + b4c
    out = minibatch_loss(mu, value, std, to64(batch), ppo_rows, coeff, perm, sign, **kw)
    out["loss"].backward()
    zero = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)
    y = A3.detach()
    dZ3 = zero(A3) * torch.where(y > 0, torch.ones_like(y), y + 1)
    return dict(dZ3=dZ3, dW4a=zero(W4a), dW4c=zero(W4c), db3=dZ3.sum(1), g_std=zero(std), g_b4a=zero(b4a),
                g_b4c=zero(b4c), kl=out["kl"].item(), surrogate=out["surrogate"].item(),
                value_loss=out["value_loss"].item(), symmetry=out["symmetry"].item())
