"""fp64 reference of the plain dense nn.Linear calls (launch_gemm with no generalised addressing: gemm9, gemm8, the
256 x 256 tile kernel and the generic 64 x 64 kernel) and of their five plain epilogues, with a per-element error bound,
the operands the tests run on and the shape tables.  Plain torch (every function follows the device of its arguments),
no kernel imported.  tests/test_dense_gemm_reference_cpu.py pins the module without a GPU, tests/test_dense_gemm_gpu.py
applies it to the kernels.

Every number comes from tests/_gemm_ref.py (G) and tests/_ln_fold_ref.py (R); none is tuned against a kernel:
    EPI_STORE_F32   G.dense (K products and the bias summed in fp32 in any order, truncating adder allowed) and one fp32
                    rounding of the result
    EPI_STORE_T     G.store on top of G.dense
    EPI_RESID_F32   resid + y: G.dense's bound plus U |resid + y| (the one fp32 addition of the epilogue)
    EPI_GELU_T      R.gelu_out_bound on G.dense's value and bound, the operand-dtype coefficient set
    EPI_GELU_F32    R.gelu_out_bound on G.dense's value and bound, the fp32 coefficient set
The generic kernel evaluates x / 2 (1 + erff(x / sqrt 2)) in both GELU epilogues (gemm.hip, common.h gelu_erf).  It is
held to the figures of the fp32 coefficient set, which was itself fitted to that function: erff is good to a few ulp, so
|gelu_erf - gelu| is a few 2^-24 max(1, |x|), at most 6e-7 at the clamp 4.75 against the 2e-6 of the set, and the product
with x is one more rounding (tests/test_gelu_epilogue_gpu.py measured 0.22 of a bound that is itself below this one).

Exact case: a in {-1, 0, 1}, w and bias in {-2 .. 2}, integer residuals.  Every partial sum is an integer of magnitude
<= 2 K + 2, exact in fp32 and, for K <= EXACT_K[dtype], in the operand dtype: whatever its summation order, a correct
kernel gives the fp64 result BIT FOR BIT in the three epilogues without a GELU."""
import math

import torch

import _gemm_ref as G
import _ln_fold_ref as R

EPI_STORE_T, EPI_STORE_F32, EPI_GELU_T, EPI_GELU_F32, EPI_RESID_F32 = 0, 1, 2, 3, 4  # include/esmk.h
EPILOGUES = (EPI_STORE_T, EPI_STORE_F32, EPI_GELU_T, EPI_GELU_F32, EPI_RESID_F32)
EPI_NAMES = {EPI_STORE_T: "store_t", EPI_STORE_F32: "store_f32", EPI_GELU_T: "gelu_t", EPI_GELU_F32: "gelu_f32",
             EPI_RESID_F32: "resid_f32"}
EXACT_EPILOGUES = (EPI_STORE_T, EPI_STORE_F32, EPI_RESID_F32)  # the GELU epilogues are held to their bound there
DTYPES = (torch.float16, torch.bfloat16)

WORKGROUPS = 256  # gemm9.hip num_workgroups9 / gemm8.hip num_workgroups on the MI355X: 256 CUs, rounded down to 8s

# (M, N, K): the smallest shapes at which each mechanism of the tiled kernels can still go wrong
EDGE_SHAPES = (
    (1, 8, 64),        # one row, the smallest N, one K tile
    (127, 264, 192),   # either side of the 128-row wave block / half-height tile; N tail of 8 past a full 256 tile;
    (128, 264, 192),   # 3 K tiles: odd for the two-buffer parity, a full cycle of the three-buffer one
    (129, 264, 192),
    (255, 136, 128),   # either side of the 256-row tile; the N tail inside the second 128-column wave block
    (257, 136, 128),
    (300, 384, 256),   # both tails (the shape of test_kernels_gpu.py)
    (130, 264, 5120),  # 80 K tiles on a clipped tile: the bound at its loosest
)
# more tiles than workgroups and at most twice as many, a single row in the last row tile, N % 256 == 8; 1 and 5 K tiles:
# the parity of both buffer schemes differs from tile to tile of a workgroup.  (M, N, K, rows of a tile)
SEAM_SHAPES = (
    (8449, 2056, 64, 256), (8449, 2056, 320, 256),  # 34 x 9 = 306 full-height tiles
    (4225, 2056, 64, 128), (4225, 2056, 320, 128),  # 34 x 9 = 306 half-height tiles
)
GENERIC_SHAPES = ((77, 33, 320), (130, 200, 96))  # N % 4 != 0; K % 64 != 0: the generic kernel alone takes them
EXACT_K = {torch.float16: 960, torch.bfloat16: 64}  # 2 K + 2 <= 2048 / 256: integers the dtype holds exactly


def is_seam(M, N, K, tile_m):
    tiles = ((M + tile_m - 1) // tile_m) * ((N + 255) // 256)
    return WORKGROUPS < tiles <= 2 * WORKGROUPS and M % tile_m == 1 and N % 256 == 8


def exact_k(K, dtype):
    """K cut to what exact_case allows"""
    return min(K, EXACT_K[dtype])


def n_tail_start(N):
    """first column of the N tail: the last, partly filled 128-column wave block"""
    return (N - 1) // 128 * 128


def last_row_block(M, rows=128):
    """first row of the clipped last block of `rows` rows"""
    return (M - 1) // rows * rows


# ---- operands ---------------------------------------------------------------------------------------------------------
def case(M, N, K, dtype, seed, device="cpu"):
    """a [M,K], w [N,K] already rounded to `dtype`, bias fp32 [N], resid fp32 [M,N].  The rows of w are scaled by a
    linspace over N (a permuted or transposed tile cannot pass) and by K^-1/2 (pre-activations of order 1, where the
    GELU bends)."""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randn(M, K, device=device, generator=g).to(dtype)
    w = (torch.randn(N, K, device=device, generator=g) * (torch.linspace(0.5, 1.5, N, device=device) / math.sqrt(K))[:, None]).to(dtype)
    bias = torch.randn(N, device=device, generator=g)
    resid = torch.randn(M, N, device=device, generator=g)
    return a, w, bias, resid


def exact_case(M, N, K, dtype, seed=0, device="cpu"):
    """small-integer operands: a in {-1, 0, 1}, w and bias in {-2 .. 2}, resid in {-8 .. 8}; K <= EXACT_K[dtype]"""
    assert 2 * K + 2 <= 2 ** (R.MANT[dtype] + 1), (K, dtype)
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randint(-1, 2, (M, K), device=device, generator=g).to(dtype)
    w = torch.randint(-2, 3, (N, K), device=device, generator=g).to(dtype)
    bias = torch.randint(-2, 3, (N,), device=device, generator=g).float()
    resid = torch.randint(-8, 9, (M, N), device=device, generator=g).float()
    y = a.double() @ w.double().T
    for t in (y, y + bias.double(), y + bias.double() + resid.double()):  # the results round-trip through the formats
        assert torch.equal(t.float().double(), t)
    for t in (y, y + bias.double()):
        assert torch.equal(t.to(dtype).double(), t)
    return a, w, bias, resid


def out_dtype(epi, dtype):
    return dtype if epi in (EPI_STORE_T, EPI_GELU_T) else torch.float32


# ---- value and bound --------------------------------------------------------------------------------------------------
def expected(epi, a, w, bias, resid, generic=False):
    """(value fp64, bound fp64) [M,N] with |kernel - value| <= bound per element.  bias: fp32 [N] or None; resid: fp32
    [M,N], read by EPI_RESID_F32 alone; generic: the 64 x 64 kernel (erff in the GELU epilogues)."""
    y, b = G.dense(a, w, bias)
    if epi == EPI_STORE_F32:
        return y, b + G.U * y.abs()
    if epi == EPI_STORE_T:
        return y, G.store(y, b, a.dtype)
    if epi == EPI_RESID_F32:
        v = resid.double() + y
        return v, b + G.U * v.abs()
    if epi == EPI_GELU_T:
        return R.gelu_out_bound(y, b, a.dtype, t16=not generic)
    if epi == EPI_GELU_F32:
        return R.gelu_out_bound(y, b, torch.float32, t16=False)
    raise ValueError(epi)


def exact_expected(epi, a, w, bias, resid):
    """the exact case's result in the output dtype (EXACT_EPILOGUES): what a correct kernel stores, bit for bit"""
    y = a.double() @ w.double().T + (0 if bias is None else bias.double())
    if epi == EPI_RESID_F32:
        y = y + resid.double()
    out = y.to(out_dtype(epi, a.dtype))
    assert torch.equal(out.double(), y)
    return out


def where(m, n, tile_m, tile_n=256):
    """which tile and 128 x 128 wave block an element lies in, for failure messages"""
    return (f"tile ({m // tile_m}, {n // tile_n}) of {tile_m} x {tile_n}, row {m % tile_m} col {n % tile_n} in it, "
            f"wave block ({m % tile_m // 128}, {n % tile_n // 128})")
