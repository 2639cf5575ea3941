"""GPU: every kernel that evaluates f32 products as six bf16 limb products is held to the
"f32-accurate" claim - the pipelined and the register-staged lgx_gemm_nt kernels, the six
lgx_gemm_tn kernels and the rollout MLP (lgx_mlp_x3_forward).

1. Single-product probe (split_products_ref.py): one operand one-hot along the reduction index, so
   every output element is one product and must satisfy |C - a b| <= 2^-21 |a b| against float64
   (derivation in split_products_ref's docstring; the exact-f32 kernel, as a control of the
   harness, meets 2^-24).  Operands are positive so that the epilogues are exact identities; outputs
   are pre-filled with NaN and every element is checked.
2. Dense accumulation: the criterion of test_gpu_gemm.test_split_bf16_is_f32_accurate (max and mean
   error against float64 within 1.25x of the exact-f32 MFMA kernel's on the same operands, every
   element within K 2^-24 sum |a b|) on the kernels production runs.

Every test prints its largest error in units of 2^-24 before it asserts.
"""
import ctypes as C

import pytest
import torch

import split_products_ref as sp
from legged_gym_amd.sim import abi
from legged_gym_amd.sim import lib as lgxlib
from test_gpu_gemm import _lib, _plain, _presplit, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPIS = {"plain": abi.GEMM_PLAIN, "bias_elu": abi.GEMM_BIAS_ELU, "delu_colsum": abi.GEMM_DELU_COLSUM,
        "delu": abi.GEMM_DELU}
DELU_Y = (1.0, -0.5, -0.75)        # ELU outputs whose ELU' is exactly 1, 0.5, 0.25


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _check(name, got, expect, bound):
    err = sp.rel_err_ulps(got, expect)
    worst = err.max().item()
    print(f"PROBE {name}: max {worst:.3f} x 2^-24 (bound {bound / sp.ULP24:g}), "
          f"{int((err * sp.ULP24 > bound).sum())} of {err.numel()} over")
    assert bool((err * sp.ULP24 <= bound).all()), f"{name}: max rel err {worst:.2f} x 2^-24 > {bound / sp.ULP24:g}"


# ---- a. lgx_gemm_nt

def _gemm_nt(A, B, epi, algo, presplit, tile_rows, Y):
    batch, M, K = A.shape
    N = B.shape[1]
    Cout = torch.full((batch, M, N), float("nan"), device=DEV)
    a = abi.LgxGemmArgs()
    a.M, a.N, a.K, a.batch, a.epi = M, N, K, batch, epi
    a.A, a.lda, a.sa = A.data_ptr(), K, M * K
    a.B, a.ldb, a.sb = B.data_ptr(), K, N * K
    a.C, a.ldc, a.sc = Cout.data_ptr(), N, M * N
    a.algo, a.tile_rows = algo, tile_rows
    keep = []
    if epi == abi.GEMM_BIAS_ELU:
        keep.append(torch.zeros(batch, N, device=DEV))
        a.bias = keep[-1].data_ptr()
    if epi in (abi.GEMM_DELU_COLSUM, abi.GEMM_DELU):
        a.Y = Y.data_ptr()
    parts = None
    if epi == abi.GEMM_DELU_COLSUM:
        parts = torch.full((_lib().lgx_gemm_partials_floats(M, N, batch),), float("nan"), device=DEV)
        a.partials = parts.data_ptr()
    if presplit:
        keep.append(_presplit(B))
        a.Bs = keep[-1].data_ptr()
    lgxlib.check(_lib().lgx_gemm_nt(C.byref(a), _stream()), "lgx_gemm_nt")
    torch.cuda.synchronize()
    if parts is not None:            # column-sum partials accumulate: not held to the product bound
        assert bool(torch.isfinite(parts).all())
    return Cout


def _nt_probe(K, onehot, epi_name, algo, presplit, tile_rows=0, bound=sp.PROBE_BOUND, M=None, N=None, seed=0):
    """lgx_gemm_nt with A (rows) or B (output columns) one-hot over k, batch 2 with distinct data."""
    g = _gen(1000 * K + 10 * tile_rows + seed)
    epi = EPIS[epi_name]
    if onehot == "A":        # M = 2K + 44: a ragged last tile, every k at two row positions; dense B
        M, N = M or 2 * K + 44, N or 256
        idx = sp.hit_index(M, K, DEV)
        vals, B = sp.operands((2, M), g, DEV), sp.operands((2, N, K), g, DEV)
        A = sp.onehot_rows(vals, idx, K)
        expect = sp.expect_rows(vals, idx, B)
    else:                    # N >= K rounded up to 128: every k; dense A
        M, N = M or 300, N or max(128, -(-K // 128) * 128)
        idx = sp.hit_index(N, K, DEV)
        vals, A = sp.operands((2, N), g, DEV), sp.operands((2, M, K), g, DEV)
        B = sp.onehot_rows(vals, idx, K)
        expect = sp.expect_rows(vals, idx, A).transpose(1, 2)
    Y = None
    if epi in (abi.GEMM_DELU_COLSUM, abi.GEMM_DELU):
        Y = torch.tensor(DELU_Y, device=DEV)[torch.randint(0, 3, (2, M, N), generator=g, device=DEV)]
        expect = expect * torch.where(Y > 0, torch.ones_like(Y), Y + 1).double()      # exact factors
    got = _gemm_nt(A.contiguous(), B.contiguous(), epi, algo, presplit, tile_rows, Y)
    _check(f"gemm_nt algo={algo} presplit={int(presplit)} K={K} pm={tile_rows} {epi_name} onehot={onehot} M={M} N={N}",
           got, expect, bound)


@pytest.mark.parametrize("onehot", ["A", "B"])
@pytest.mark.parametrize("epi", ["plain", "bias_elu", "delu_colsum"])
@pytest.mark.parametrize("K", [512, 36])
def test_probe_gemm_nt_exact_f32_control(gpu, K, epi, onehot):
    """The exact-f32 MFMA kernel through the same probe: one rounding of a*b, 2^-24."""
    _nt_probe(K, onehot, epi, abi.GEMM_ALGO_F32, False, bound=sp.F32_BOUND)


@pytest.mark.parametrize("onehot", ["A", "B"])
@pytest.mark.parametrize("epi", ["plain", "bias_elu", "delu_colsum"])
@pytest.mark.parametrize("K", [512, 36])
def test_probe_gemm_nt_register_staged(gpu, K, epi, onehot):
    """gemm_nt_x3_kernel<.., BS=false>: both operands split in the kernel (K 36: a 4-wide tail stage)."""
    _nt_probe(K, onehot, epi, abi.GEMM_ALGO_SPLIT_BF16, False)


@pytest.mark.parametrize("onehot", ["A", "B"])
@pytest.mark.parametrize("epi", ["plain", "bias_elu", "delu_colsum"])
def test_probe_gemm_nt_register_staged_presplit(gpu, epi, onehot):
    """gemm_nt_x3_kernel<.., BS=true>: a pre-split B with K % 32 != 0."""
    _nt_probe(36, onehot, epi, abi.GEMM_ALGO_SPLIT_BF16, True)


@pytest.mark.parametrize("onehot", ["A", "B"])
@pytest.mark.parametrize("epi", ["plain", "bias_elu", "delu_colsum", "delu"])
@pytest.mark.parametrize("pm", [128, 256])
@pytest.mark.parametrize("K", [128, 256, 512, 96])
def test_probe_gemm_nt_pipelined(gpu, K, pm, epi, onehot):
    """gemm_nt_x3p_kernel: 4 epilogues x K unroll {128, 256, 512, runtime 96} x tile height {128, 256}."""
    _nt_probe(K, onehot, epi, abi.GEMM_ALGO_SPLIT_BF16, True, tile_rows=pm)


@pytest.mark.parametrize("epi", ["bias_elu", "delu"])
@pytest.mark.parametrize("pm", [128, 256])
def test_probe_gemm_nt_pipelined_several_tiles_per_workgroup(gpu, pm, epi):
    """24,576 rows: every persistent workgroup walks several tiles, so the deferred epilogue of one
    tile runs inside the next tile's slots."""
    _nt_probe(128, "A", epi, abi.GEMM_ALGO_SPLIT_BF16, True, tile_rows=pm, M=24576, N=256)


# ---- b. lgx_gemm_tn

TN_KERNELS = {                      # (LGX_TN_RING, LGX_TN_WS, R): the switches are read per call
    "ring256": (None, None, 256), "ring128": (None, None, 128), "ring128_r384": (None, None, 384),
    "ws256": ("0", "2", 256), "ws128": ("0", "1", 128), "x3_8": ("0", "0", 256), "x3_4": ("0", "0", 128),
}


def _tn_env(monkeypatch, kernel):
    ring, ws, R = TN_KERNELS[kernel]
    for name, v in (("LGX_TN_RING", ring), ("LGX_TN_WS", ws)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    return R


def _gemm_tn(A, B, S, Cc):
    batch, M, R = A.shape
    ldb = B.shape[2]
    Cout = torch.full((batch, S, R, Cc), float("nan"), device=DEV)
    cs = torch.full((batch, S, R), float("nan"), device=DEV)
    a = abi.LgxGemmTnArgs()
    a.M, a.R, a.Cc, a.slices, a.batch = M, R, Cc, S, batch
    a.A, a.lda, a.sa = A.data_ptr(), R, M * R
    a.B, a.ldb, a.sb = B.data_ptr(), ldb, M * ldb
    a.C, a.ldc, a.colsum = Cout.data_ptr(), Cc, cs.data_ptr()
    lgxlib.check(_lib().lgx_gemm_tn(C.byref(a), _stream()), "lgx_gemm_tn")
    torch.cuda.synchronize()
    return Cout, cs


@pytest.mark.parametrize("onehot", ["A", "B"])
@pytest.mark.parametrize("Cc,ldb", [(128, 128), (235, 256)])
@pytest.mark.parametrize("kernel", list(TN_KERNELS))
def test_probe_gemm_tn(gpu, monkeypatch, kernel, Cc, ldb, onehot):
    """lgx_gemm_tn (reduction over the rows of a slice): one nonzero per column and slice in A (dense
    B) or in B (dense A).  320 rows in 2 slices: 160 rows = 10 ring stages, every row of a slice hit;
    the padding columns of B (235 -> 256) hold data that must not reach C.  With A one-hot the column
    sums are that one value, bit for bit."""
    R = _tn_env(monkeypatch, kernel)
    M, S, batch = 320, 2, 2
    Ms = M // S
    g = _gen(R + Cc + (onehot == "B"))
    if onehot == "A":
        idx = sp.slice_row_index(R, Ms, batch, S, DEV)
        vals, B = sp.operands((batch, S, R), g, DEV), sp.operands((batch, M, ldb), g, DEV)
        A = sp.onehot_slices(vals, idx, Ms)
        expect = sp.expect_slices(vals, idx, B[..., :Cc], Ms)
    else:
        idx = sp.slice_row_index(ldb, Ms, batch, S, DEV)
        vals, A = sp.operands((batch, S, ldb), g, DEV), sp.operands((batch, M, R), g, DEV)
        B = sp.onehot_slices(vals, idx, Ms)
        expect = sp.expect_slices(vals, idx, A, Ms).transpose(2, 3)[..., :Cc]
    got, cs = _gemm_tn(A.contiguous(), B.contiguous(), S, Cc)
    if onehot == "A":
        assert torch.equal(cs, vals), "colsum of a one-hot column is its nonzero"
    else:
        assert bool(torch.isfinite(cs).all())
    _check(f"gemm_tn {kernel} R={R} Cc={Cc} onehot={onehot}", got, expect, sp.PROBE_BOUND)


# ---- c. lgx_mlp_x3_forward

def _mlp_desc(d, x, y, dims, weights, keep):
    """Fill one lgx_mlp_x3_desc: ELU hidden layers, zero biases, weight images from lgx_mlp_x3_split."""
    lib = _lib()
    d.x, d.y, d.rows, d.nl, d.act = x.data_ptr(), y.data_ptr(), x.shape[0], len(weights), 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i, w in enumerate(weights):
        assert tuple(w.shape) == (dims[i + 1], dims[i]) and w.is_contiguous()
        wl = torch.full((int(lib.lgx_mlp_x3_weight_elems(dims[i + 1], dims[i])),), -1, dtype=torch.int16, device=DEV)
        lgxlib.check(lib.lgx_mlp_x3_split(C.c_void_p(w.data_ptr()), dims[i + 1], dims[i], C.c_void_p(wl.data_ptr()),
                                          _stream()), "lgx_mlp_x3_split")
        b = torch.zeros(dims[i + 1], device=DEV)
        keep += [wl, b]
        d.weights[i], d.biases[i] = wl.data_ptr(), b.data_ptr()


def _mlp_x3(nets):
    """One lgx_mlp_x3_forward launch of 1 or 2 networks (x, dims, weights); the f32 output rows."""
    lib = _lib()
    d = (abi.LgxMlpX3Desc * len(nets))()
    keep, ys = [], []
    for i, (x, dims, weights) in enumerate(nets):
        ys.append(torch.full((x.shape[0], dims[-1]), float("nan"), device=DEV))
        _mlp_desc(d[i], x, ys[-1], dims, weights, keep)
    assert lib.lgx_mlp_x3_lds_bytes(d, len(nets)) > 0
    lgxlib.check(lib.lgx_mlp_x3_forward(d, len(nets), _stream()), "lgx_mlp_x3_forward")
    torch.cuda.synchronize()
    return ys


def _one_layer(k_in, n_out, onehot, g):
    if onehot == "x":         # rows = 2 k_in + 5: ragged 32-row tiles, every k at two row positions
        rows = 2 * k_in + 5
        idx = sp.hit_index(rows, k_in, DEV)
        vals, W = sp.operands((rows,), g, DEV), sp.operands((n_out, k_in), g, DEV)
        return sp.onehot_rows(vals, idx, k_in), [W], sp.expect_rows(vals, idx, W)
    rows = 69                 # dense x; W has one nonzero per output row
    idx = sp.hit_index(n_out, k_in, DEV)
    vals, x = sp.operands((n_out,), g, DEV), sp.operands((rows, k_in), g, DEV)
    return x, [sp.onehot_rows(vals, idx, k_in)], sp.expect_rows(vals, idx, x).t()


def _two_layers(k_in, H, n_out, g, off=0):
    """x one-hot over k, W1[j][k] = (j == (k + off) % H): h = ELU(x W1^T) is x's nonzero moved to
    column (k + off) % H, exactly; W2 dense: y[r][o] = x[r] * W2[o][(k(r) + off) % H] through the
    epilogue's limb split."""
    rows = 2 * k_in + 5
    idx = sp.hit_index(rows, k_in, DEV)
    vals, W2 = sp.operands((rows,), g, DEV), sp.operands((n_out, H), g, DEV)
    W1 = (torch.arange(H, device=DEV)[:, None] == (torch.arange(k_in, device=DEV)[None, :] + off) % H).float()
    return sp.onehot_rows(vals, idx, k_in), [W1, W2], sp.expect_rows(vals, (idx + off) % H, W2)


@pytest.mark.parametrize("k_in,n_out,onehot", [(235, 12, "x"), (48, 1, "x"), (512, 512, "x"), (7, 5, "x"),
                                               (235, 12, "W"), (48, 1, "W"), (512, 512, "W"), (7, 5, "W"),
                                               (235, 300, "W"), (48, 50, "W"), (7, 9, "W")])
def test_probe_mlp_x3_one_layer(gpu, k_in, n_out, onehot):
    """nl = 1, zero bias: a bare GEMM from the staged input's limb image to f32 rows.  x one-hot over k
    (dense weight image: every (n, k) of it), or dense x with one nonzero per weight row (n_out >=
    k_in: every k of the staged input)."""
    x, ws, expect = _one_layer(k_in, n_out, onehot, _gen(k_in + n_out))
    (y,) = _mlp_x3([(x, (k_in, n_out), ws)])
    _check(f"mlp_x3 1 layer {k_in}->{n_out} onehot={onehot}", y, expect, sp.PROBE_BOUND)


@pytest.mark.parametrize("n_out", [12, 1])
@pytest.mark.parametrize("k_in,H,off", [(256, 512, 0), (256, 512, 256), (135, 128, 0), (40, 33, 0)])
def test_probe_mlp_x3_two_layers(gpu, k_in, H, off, n_out):
    """nl = 2 with ELU: the first layer's epilogue splits its activations into the second layer's LDS
    limb image; every k of layer 2 is hit (H 512: two 512-wide images exceed the LDS, so a 256-wide
    input reaches the lower and, with off = 256, the upper half).  Two chained products: 2 * 2^-21."""
    x, ws, expect = _two_layers(k_in, H, n_out, _gen(H + n_out + off), off)
    (y,) = _mlp_x3([(x, (k_in, H, n_out), ws)])
    _check(f"mlp_x3 2 layers {k_in}->{H}->{n_out} off={off}", y, expect, 2 * sp.PROBE_BOUND)


def test_probe_mlp_x3_two_networks(gpu):
    """Both networks of one launch (the rollout's actor + critic form), the same number of rows."""
    g = _gen(77)
    xa, wa, ea = _two_layers(235, 128, 12, g)
    rows = xa.shape[0]
    idx = sp.hit_index(rows, 48, DEV)
    vals, Wc = sp.operands((rows,), g, DEV), sp.operands((1, 48), g, DEV)
    ya, yc = _mlp_x3([(xa, (235, 128, 12), wa), (sp.onehot_rows(vals, idx, 48), (48, 1), [Wc])])
    _check("mlp_x3 pair, net 0 235->128->12", ya, ea, 2 * sp.PROBE_BOUND)
    _check("mlp_x3 pair, net 1 48->1", yc, sp.expect_rows(vals, idx, Wc), sp.PROBE_BOUND)


# ---- 2. dense accumulation against the exact-f32 MFMA kernel
#
# Measured on an MI355X, split-bf16 error / exact-f32 error against float64 (spread 0 | spread 12):
#   at the seeds of these tests   max: x3p 0.72-0.90 | 0.84-1.13, tn 0.70-0.81 | 0.81-0.82, mlp 1.05 | 0.64
#                                mean: 0.84 | 0.90 for every kernel (6 accumulator roundings per 16 k against 16)
#   over five other seeds         max: x3p 0.60-1.03 | 0.50-1.04, tn 0.75-1.01 | 0.64-1.69, mlp 0.62-0.89 | 0.64-1.15
#                                mean: 0.835-0.845 | 0.892-0.903
# The mean ratio is the sharp figure (the exact-f32 kernel's own mean moves by 0.2-2.7 % from seed to
# seed); the max is one extreme element of 10^6 (the exact-f32 kernel's own max moves by 1.10-2.05x
# over the same five seeds), so at another seed a kernel this accurate can exceed 1.25 on it.  Both
# keep the project's 1.25 here: no kernel needed more at these seeds.

MARGIN = 1.25


def _dense_operands(shape_a, shape_b, spread, seed):
    g = _gen(seed)
    A, B = torch.randn(*shape_a, device=DEV, generator=g), torch.randn(*shape_b, device=DEV, generator=g)
    if spread:
        A = A * torch.exp2(torch.randint(-spread, spread + 1, A.shape, device=DEV, generator=g).float())
        B = B * torch.exp2(torch.randint(-spread, spread + 1, B.shape, device=DEV, generator=g).float())
    return A, B


def _dense_errors(name, got, A, B):
    """got against float64 A B^T ([batch, M, K] x [batch, N, K]), next to the exact-f32 kernel's errors."""
    K = A.shape[2]
    ref = torch.bmm(A.double(), B.double().transpose(1, 2))
    scale = torch.bmm(A.double().abs(), B.double().abs().transpose(1, 2))
    e32 = (_plain(A, B, abi.GEMM_ALGO_F32).double() - ref).abs()
    esp = (got.double() - ref).abs()
    out = {"max": esp.max().item() / e32.max().item(), "mean": esp.mean().item() / e32.mean().item(),
           "e32_max": e32.max().item(), "e32_mean": e32.mean().item(),
           "elementwise": bool((esp <= K * 2.0 ** -24 * scale).all())}
    print(f"DENSE {name}: max ratio {out['max']:.4f} mean ratio {out['mean']:.4f} "
          f"(f32 max {out['e32_max']:.4e} mean {out['e32_mean']:.4e})")
    return out


def _assert_dense(name, got, A, B):
    r = _dense_errors(name, got, A, B)
    assert r["max"] <= MARGIN, f"{name}: max error {r['max']:.3f}x the exact-f32 kernel's"
    assert r["mean"] <= MARGIN, f"{name}: mean error {r['mean']:.3f}x the exact-f32 kernel's"
    assert r["elementwise"], f"{name}: an element beyond K 2^-24 sum |a b|"


def _dense_nt(spread, pm, seed=None):
    A, B = _dense_operands((2, 2048, 512), (2, 256, 512), spread, 17 + spread + pm if seed is None else seed)
    got = _gemm_nt(A, B, abi.GEMM_PLAIN, abi.GEMM_ALGO_SPLIT_BF16, True, pm, None)
    return f"gemm_nt x3p pm={pm} spread={spread}", got, A, B


def _dense_tn(spread, R, seed=None):
    """lgx_gemm_tn against lgx_gemm_nt's exact-f32 kernel on the transposed slices."""
    M, S, Cc = 1024, 2, 256
    A, B = _dense_operands((2, M, R), (2, M, Cc), spread, 29 + spread + R if seed is None else seed)
    got, _ = _gemm_tn(A, B, S, Cc)
    At = A.view(2 * S, M // S, R).transpose(1, 2).contiguous()        # [z s, R, Ms]
    Bt = B.view(2 * S, M // S, Cc).transpose(1, 2).contiguous()       # [z s, Cc, Ms]
    return got.view(2 * S, R, Cc), At, Bt


def _dense_mlp(spread, seed=None):
    x, W = _dense_operands((1, 1000, 512), (1, 512, 512), spread, 41 + spread if seed is None else seed)
    (y,) = _mlp_x3([(x[0], (512, 512), [W[0]])])
    return "mlp_x3 1 layer 512->512", y[None], x, W


@pytest.mark.parametrize("pm", [128, 256])
@pytest.mark.parametrize("spread", [0, 12])
def test_dense_gemm_nt_pipelined_is_f32_accurate(gpu, spread, pm):
    """gemm_nt_x3p_kernel, both tile heights.  Measured max / mean ratio: 0.90 / 0.84 and 0.72 / 0.84 (spread 0),
    0.84 / 0.90 and 1.13 / 0.90 (spread 12) for 128- and 256-row tiles."""
    _assert_dense(*_dense_nt(spread, pm))


@pytest.mark.parametrize("kernel", ["ring256", "ring128", "ws256", "ws128", "x3_8", "x3_4"])
@pytest.mark.parametrize("spread", [0, 12])
def test_dense_gemm_tn_is_f32_accurate(gpu, monkeypatch, spread, kernel):
    """The six lgx_gemm_tn kernels against the exact-f32 lgx_gemm_nt on the transposed slices.  Measured max /
    mean ratio: 0.81 / 0.84 (256-row kernels) and 0.70 / 0.84 (128-row), with spread 12 0.82 / 0.90 and 0.81 / 0.90."""
    R = _tn_env(monkeypatch, kernel)
    _assert_dense(f"gemm_tn {kernel} spread={spread}", *_dense_tn(spread, R))


@pytest.mark.parametrize("spread", [0, 12])
def test_dense_mlp_x3_is_f32_accurate(gpu, spread):
    """lgx_mlp_x3_forward as one 512 -> 512 layer.  Measured max / mean ratio: 1.05 / 0.84, with spread 12 0.64 / 0.90."""
    name, got, A, B = _dense_mlp(spread)
    _assert_dense(f"{name} spread={spread}", got, A, B)
