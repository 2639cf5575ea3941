"""Float64 numpy statement of the Distillation update (rsl_rl 2.x `Distillation`, loss_type "mse"),
independent of torch autograd and of the kernels: the reference of tests/test_distillation.py and
tests/test_gpu_distillation.py.

A student is a list of (W [out, in], b [out]) pairs: ELU (alpha 1) between the layers, none after
the last.  One chunk is `g` consecutive steps of N rows; its loss is sum_t mean_{N, A}
(student(obs_t) - target_t)^2, so d loss / d mu[r][j] = 2 (mu - target) / (N A) for every row of
the chunk (the scale is 1 / (N A), not 1 / (g N A)).
"""
import numpy as np


def forward(params, x):
    """-> (mu, the hidden layers' ELU outputs)"""
    ys = []
    for W, b in params[:-1]:
        z = x @ W.T + b
        x = np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
        ys.append(x)
    W, b = params[-1]
    return x @ W.T + b, ys


def head(y3, W4, b4, target, scale):
    """The narrow end alone (what lgx_bc_loss_bwd computes) -> dict(dz3, dW4, db4, db3, sumsq)."""
    y3, W4, b4, target = (np.asarray(a, np.float64) for a in (y3, W4, b4, target))
    d = y3 @ W4.T + b4 - target
    dmu = 2.0 * scale * d
    dz3 = (dmu @ W4) * np.where(y3 > 0, 1.0, y3 + 1.0)
    return dict(dz3=dz3, dW4=dmu.T @ y3, db4=dmu.sum(0), db3=dz3.sum(0), sumsq=float((d * d).sum()))


def chunk_loss_grad(params, obs, target):
    """obs [g, N, W], target [g, N, A] -> (chunk loss, [l_t], [(dW, db)] in layer order)"""
    params = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in params]
    g, N, _ = obs.shape
    A = target.shape[-1]
    x = np.asarray(obs, np.float64).reshape(g * N, -1)
    t = np.asarray(target, np.float64).reshape(g * N, A)
    mu, ys = forward(params, x)
    d = mu - t
    steps = [float((d[i * N:(i + 1) * N] ** 2).mean()) for i in range(g)]
    dz = 2.0 * d / (N * A)
    grads = []
    acts = [x] + ys
    for k in range(len(params) - 1, -1, -1):
        grads.append((dz.T @ acts[k], dz.sum(0)))
        if k:
            y = acts[k]
            dz = (dz @ params[k][0]) * np.where(y > 0, 1.0, y + 1.0)   # ELU' from the output
    return sum(steps), steps, grads[::-1]


def update(params, obs, target, gradient_length, epochs, lr, max_grad_norm=None, betas=(0.9, 0.999), eps=1e-8):
    """A whole update from a fresh Adam state: obs [T, N, W], target [T, N, A] ->
    (the stepped params, mean_t l_t over epochs x T).  clip_grad_norm_ as torch (coef =
    min(max_norm / (norm + 1e-6), 1)) when max_grad_norm is truthy; torch.optim.Adam's step."""
    params = [(np.array(W, np.float64), np.array(b, np.float64)) for W, b in params]
    m = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    v = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    T = obs.shape[0]
    losses, step = [], 0
    for _ in range(epochs):
        for c in range(T // gradient_length):
            sl = slice(c * gradient_length, (c + 1) * gradient_length)
            _, steps, grads = chunk_loss_grad(params, obs[sl], target[sl])
            losses += steps
            if max_grad_norm:
                norm = np.sqrt(sum((gw ** 2).sum() + (gb ** 2).sum() for gw, gb in grads))
                coef = min(max_grad_norm / (norm + 1e-6), 1.0)
                grads = [(gw * coef, gb * coef) for gw, gb in grads]
            step += 1
            bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
            new = []
            for (W, b), (gw, gb), (mw, mb), (vw, vb) in zip(params, grads, m, v):
                out = []
                for p, gr, mm, vv in ((W, gw, mw, vw), (b, gb, mb, vb)):
                    mm *= betas[0]
                    mm += (1 - betas[0]) * gr
                    vv *= betas[1]
                    vv += (1 - betas[1]) * gr * gr
                    out.append(p - (lr / bc1) * mm / (np.sqrt(vv) / np.sqrt(bc2) + eps))
                new.append(tuple(out))
            params = new
    return params, float(np.mean(losses))
