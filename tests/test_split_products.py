"""CPU: the single-product probe of tests/test_gpu_split_products.py without a kernel - the emulated
six-product sum meets the derived bound, the emulation with one order-2 product left out (or the
third limb of a neighbouring element) misses it on most elements, and the one-hot generators hit
every reduction index at the shapes the GPU tests use."""
import pytest
import torch

import split_products_ref as sp

N_SAMPLES = 1 << 20      # >= 1M


@pytest.fixture(scope="module")
def pairs():
    gen = torch.Generator().manual_seed(1)
    out = {}
    for spread in (0, 12):
        a, b = sp.operands((N_SAMPLES,), gen, spread=spread), sp.operands((N_SAMPLES,), gen, spread=spread)
        out[spread] = (a, b, a.double() * b.double())
    return out


@pytest.mark.parametrize("spread", [0, 12])
def test_emulated_six_products_meet_the_bound(pairs, spread):
    a, b, ref = pairs[spread]
    err = sp.rel_err_ulps(sp.six_products(a, b), ref)
    print(f"six products, spread {spread}: max {err.max().item():.2f} mean {err.mean().item():.3f} x 2^-24")
    assert err.max().item() * sp.ULP24 <= sp.PROBE_BOUND
    # a plain f32 product: the control bound of the exact-f32 kernel
    assert sp.rel_err_ulps(a * b, ref).max().item() * sp.ULP24 <= sp.F32_BOUND


def test_limbs_reproduce_f32_exactly(pairs):
    a = pairs[12][0]
    x0, x1, x2 = sp.limbs(a)
    assert torch.equal(x0.double() + x1.double() + x2.double(), a.double())
    assert bool((x1.abs() <= 2.0 ** -8 * x0.abs()).all()) and bool((x2.abs() <= 2.0 ** -8 * x1.abs()).all())


@pytest.mark.parametrize("spread", [0, 12])
@pytest.mark.parametrize("fault", sp.ORDER2 + ("neighbour",))
def test_bound_catches_a_lost_limb_product(pairs, spread, fault):
    a, b, ref = pairs[spread]
    got = sp.six_products(a, b, third_from_neighbour=True) if fault == "neighbour" else sp.six_products(a, b, drop=fault)
    err = sp.rel_err_ulps(got, ref)
    over = (err * sp.ULP24 > sp.PROBE_BOUND).float().mean().item()
    print(f"{fault}, spread {spread}: {100 * over:.1f}% over the bound, max {err.max().item():.0f} "
          f"mean {err.mean().item():.1f} x 2^-24")
    assert over > 0.5


NT_K = (512, 256, 128, 96, 36)
MLP_K = (235, 48, 512, 7, 135, 40)


@pytest.mark.parametrize("K", sorted(set(NT_K + MLP_K)))
def test_hit_index_covers_every_k(K):
    for count in (2 * K + 44, 2 * K + 5):          # one-hot rows of lgx_gemm_nt's A / the MLP's input
        idx = sp.hit_index(count, K)
        assert int(idx.min()) == 0 and int(idx.max()) == K - 1
        assert int(torch.bincount(idx, minlength=K).min()) >= 2
        # the two hits of a k sit at different row positions of a 128-row tile
        first, second = idx[:K], idx[K:2 * K]
        pos2 = torch.empty(K, dtype=torch.long)
        pos2[second] = torch.arange(K, 2 * K)
        pos1 = torch.empty(K, dtype=torch.long)
        pos1[first] = torch.arange(K)
        assert bool(((pos2 - pos1) % 128 != 0).all())
    n_cols = max(128, -(-K // 128) * 128)            # one-hot columns of B: N >= K, a multiple of 128
    assert int(torch.bincount(sp.hit_index(n_cols, K), minlength=K).min()) >= 1


@pytest.mark.parametrize("ncols", [128, 235, 256, 384])
def test_slice_row_index_covers_every_row(ncols):
    Ms, batch, S = 160, 2, 2
    idx = sp.slice_row_index(ncols, Ms, batch, S)
    assert idx.shape == (batch, S, ncols) and int(idx.min()) >= 0 and int(idx.max()) < Ms
    assert int(torch.bincount(idx.flatten(), minlength=Ms).min()) >= 1      # over the batch and slices
    if ncols >= Ms:
        for z in range(batch):
            for s in range(S):
                assert int(torch.bincount(idx[z, s], minlength=Ms).min()) >= 1


def test_expectations_are_the_float64_products():
    """The gathered single products equal float64 matrix products of the one-hot operands."""
    gen = torch.Generator().manual_seed(3)
    K, M, N = 36, 2 * 36 + 44, 128
    idx = sp.hit_index(M, K)
    vals, dense = sp.operands((2, M), gen), sp.operands((2, N, K), gen)
    A = sp.onehot_rows(vals, idx, K)
    assert int((A != 0).sum()) == 2 * M
    assert torch.equal(sp.expect_rows(vals, idx, dense), torch.bmm(A.double(), dense.double().transpose(1, 2)))
    Ms, S, R, Cc = 160, 2, 128, 235
    ridx = sp.slice_row_index(R, Ms, 2, S)
    v, B = sp.operands((2, S, R), gen), sp.operands((2, S * Ms, Cc), gen)
    A = sp.onehot_slices(v, ridx, Ms)
    assert int((A != 0).sum()) == 2 * S * R
    ref = torch.einsum("zsmn,zsmc->zsnc", A.double().view(2, S, Ms, R), B.double().view(2, S, Ms, Cc))
    assert torch.equal(sp.expect_slices(v, ridx, B, Ms), ref)
