"""Single-product probe of the split-bf16 ("f32-accurate") kernels: operand and one-hot generators,
the float64 expectation and a torch emulation of the six-limb-product sum.

The probe.  One operand of a GEMM is made one-hot along the reduction index, so every output
element is ONE product a*b and every other summand an exact zero (0 * finite, limbs of 0 are 0):
nothing accumulates, and an output that is off by more than the bound below has lost a limb
product, or read a limb from the wrong slot, at exactly that (row, column, k) position.

The bound.  a = a0 + a1 + a2 with RNE bf16 limbs (8 significant bits): a0 = bf16(a),
a1 = bf16(a - a0), a2 = bf16(a - a0 - a1); both subtractions are exact in f32.
  * limbs: |a - a0| <= 2^-9 * 2^e <= 2^-8 |a0| (half a bf16 ulp), so |a1| <= 2^-8 |a0|,
    |a2| <= 2^-8 |a1| <= 2^-16 |a0|, |a0| <= (1 + 2^-8) |a|;
  * split residue: a - a0 is a multiple of ulp_f32(a) = 2^(e-23) below 2^(e-8): 16 bits; after a1
    it is a multiple of 2^(e-23) of at most 2^(e-16): it fits the 8 bits of a2, so the three limbs
    reproduce a normal f32 exactly (the issue allowed 2^-24 |a| per operand; it is 0, and
    test_split_bf16_limbs holds the kernels' split to 2^-26);
  * dropped products: |a1 b2| + |a2 b1| + |a2 b2| <= (2 * 2^-24 + 2^-32) |a0 b0| <= 2.04 * 2^-24 |a b|;
  * accumulation: every bf16 x bf16 product is exact in f32 (16 bits); the six products enter an
    f32 accumulator that starts at an exact zero.  Whatever the order, the first add is exact and
    each of the other five rounds a partial sum of at most ~|a b|: <= 5 * 2^-24 |a b| with a
    round-to-nearest accumulator.  An accumulator that truncates (2^-23 per add) stays below that
    when the small products come first, the order all these kernels document: the five partial
    sums before a0 b0 are <= 2^-7 |a b| (5 * 2^-30), and only the last add costs 2^-23 |a b|.
  Total <= (2.04 + 5) * 2^-24 = 7.04 * 2^-24, rounded up to 8 * 2^-24 = 2^-21 = PROBE_BOUND.
Losing one order-2 product instead costs up to 2^-16 |a b| (256 * 2^-24), typically 30 * 2^-24:
test_split_products.py shows on the emulation that the bound separates the two.

The exact-f32 kernel (v_mfma_f32 fmaf chain) meets F32_BOUND = 2^-24, the one rounding of a*b.
"""
import torch

PROBE_BOUND = 2.0 ** -21
F32_BOUND = 2.0 ** -24
ULP24 = 2.0 ** -24            # errors are reported in this unit
ORDER2 = ("a0b2", "a1b1", "a2b0")


def operands(shape, gen, device="cpu", spread=12):
    """Positive f32 operands with full mantissas: |randn| (at least 2^-20) * 2^randint[-spread, spread]."""
    v = torch.randn(*shape, generator=gen, device=device).abs().clamp_min(2.0 ** -20)
    if spread:
        v = v * torch.exp2(torch.randint(-spread, spread + 1, shape, generator=gen, device=device).float())
    return v


def hit_index(count, K, device="cpu"):
    """k(i) for i < count: i-th row's (column's) nonzero position.  Passes over 0 .. K-1, each pass
    shifted by 5, so with count >= 2K every k occurs at two different positions i mod 128."""
    i = torch.arange(count, device=device)
    return (i + 5 * torch.div(i, K, rounding_mode="floor")) % K


def slice_row_index(ncols, Ms, batch, S, device="cpu"):
    """[batch, S, ncols]: the row (within its slice of Ms rows) of column n's nonzero in slice s of
    batch entry z; consecutive (z, s) continue the pass, so every row of a slice is hit."""
    n = torch.arange(ncols, device=device)[None, None, :]
    zs = (torch.arange(batch, device=device)[:, None] * S + torch.arange(S, device=device)[None, :])[..., None]
    return (n + zs * ncols) % Ms


def onehot_rows(vals, idx, K):
    """[..., M] values -> [..., M, K] with row m's only nonzero vals[..., m] at column idx[m]."""
    out = torch.zeros(*vals.shape, K, dtype=vals.dtype, device=vals.device)
    out.scatter_(-1, idx.expand(vals.shape).unsqueeze(-1), vals.unsqueeze(-1))
    return out


def onehot_slices(vals, idx, Ms):
    """[batch, S, n] values, idx [batch, S, n] -> [batch, S * Ms, n] with column n's only nonzero of
    slice s at row s * Ms + idx[z, s, n]."""
    batch, S, n = vals.shape
    out = torch.zeros(batch, S, Ms, n, dtype=vals.dtype, device=vals.device)
    out.scatter_(2, idx.unsqueeze(2), vals.unsqueeze(2))
    return out.view(batch, S * Ms, n)


def expect_rows(vals, idx, dense):
    """float64 vals[..., m] * dense[..., n, idx[m]] -> [..., m, n]: the product of a one-hot-rows operand
    (onehot_rows(vals, idx, K)) with dense^T, dense = [..., n, K]."""
    return vals.double().unsqueeze(-1) * dense.double()[..., idx].transpose(-1, -2)


def expect_slices(vals, idx, dense, Ms):
    """float64 [batch, S, n, c] = vals[z, s, n] * dense[z, s * Ms + idx[z, s, n], c]: onehot_slices^T dense
    per slice."""
    batch, S, n = vals.shape
    d = dense.double().reshape(batch, S, Ms, -1)
    rows = torch.gather(d, 2, idx.unsqueeze(-1).expand(batch, S, n, d.shape[-1]))
    return vals.double().unsqueeze(-1) * rows


def rel_err_ulps(C, expect):
    """|C - expect| / |expect| per element in units of 2^-24 (inf where C is not finite)."""
    e = (C.double() - expect).abs() / expect.abs()
    return torch.where(torch.isfinite(C), e, torch.full_like(e, float("inf"))) / ULP24


def limbs(x):
    """The three RNE bf16 limbs of f32 x, as f32."""
    x0 = x.to(torch.bfloat16).float()
    r = x - x0
    x1 = r.to(torch.bfloat16).float()
    x2 = (r - x1).to(torch.bfloat16).float()
    return x0, x1, x2


def six_products(a, b, drop=None, third_from_neighbour=False):
    """Emulation of one split-bf16 product in f32: the six limb products of order <= 2, the small ones
    first, summed in an f32 (round-to-nearest) accumulator.  drop: one of ORDER2 left out;
    third_from_neighbour: a's third limb taken from the next element (a wrong fragment slot)."""
    a0, a1, a2 = limbs(a)
    b0, b1, b2 = limbs(b)
    if third_from_neighbour:
        a2 = torch.roll(a2, 1, -1)
    acc = torch.zeros_like(a)
    for name, p in (("a0b2", a0 * b2), ("a1b1", a1 * b1), ("a2b0", a2 * b0), ("a0b1", a0 * b1), ("a1b0", a1 * b0),
                    ("a0b0", a0 * b0)):
        if name != drop:
            acc = acc + p
    return acc
