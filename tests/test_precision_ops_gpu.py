"""The kernels the precision modes (esmk_config.weight_split 1-4: f16x2, f16x2a, f16x2v, f16x3) are built from, one
launch at a time against fp64 — whole-model runs assert nothing tighter than the 1e-3 the modes promise, which a zero or
misplaced `lo` term, a wrong third slot, a spread index wrong for one head, a column clamp off by one or a dead GELU
clamp branch all survive on a 3-layer model.

    * gemm32.hip (esmk_op_linear_f32): the exact-fp32 MFMA linear of the LM head, row / column clamps, strides, GELU;
    * the weight images (esmk_op_split_weight_ex): parts 1 / 2 / 3, identity and head-spreading maps, bit for bit;
    * every form of the LayerNorm launch (esmk_op_layernorm_ex): hi | hi | lo rows, ldy, row_keep + row map, eps;
    * the f16x3 product: LayerNorm rows x parts-3 image through the plain GEMM over K' = 3 K;
    * gemm9's hi | hi | lo GELU epilogue (esmk_op_linear_gelu_x3).

References are plain torch in fp64, written here.  Every output buffer is pre-filled with a sentinel (NaN for fp32, the
bit pattern 0x7bff for 16-bit types) and carries one spare row; everything outside the specified footprint must still
hold the sentinel afterwards (padding columns, the gaps head spreading leaves, the spare row).

Bounds are a-priori: u = 2^-24, a K-term fp32 dot product plus bias is within (K + 2) u (|A| |W|^T + |bias|) of the exact
one; GELU widens that by max |gelu'| = 1.13.  What was MEASURED on an MI355X (printed by every test, `pytest -s`):

    test_linear_f32 (with bias / without), error as a fraction of the bound; erff = max error of torch's fp32 gelu on the
    kernel's pre-activations in units of u max(1, |x|) (the kernel is allowed 4x that and used exactly 1x in every case:
    it evaluates the same expression as torch):
        (M, N, K)           plain            erff measured    gelu
        (1, 33, 32)         0.026 / 0.027    0.69 / 0.71 u    0.024 / 0.026
        (129, 33, 96)       0.026 / 0.029    1.65 / 1.81 u    0.024 / 0.028
        (128, 64, 32)       0.084 / 0.084    1.83 / 1.82 u    0.070 / 0.073
        (200, 65, 320)      0.011 / 0.012    1.72 / 1.81 u    0.010 / 0.011
        (300, 1280, 1280)   0.004 / 0.004    1.89 / 2.04 u    0.003 / 0.003
    LayerNorm forms: y32 within 2.1e-7 .. 6.4e-7 of fp64 in every case (tolerance 2e-5); eps 1e-12 against 1e-5 scales the
    rows by 30.5 .. 32.7.
    test_f16x3_product (store / residual epilogue): fraction of the accumulation bound; normalised error against the
    unrounded operands of the x3 product and of plain fp16 operands, and their ratio (asserted >= 8):
        (256, 256, 64)      0.023 / 0.020    3.2e-7 vs 2.3e-4 (724 x) / 2.4e-7 vs 1.8e-4 (759 x)
        (300, 264, 192)     0.007 / 0.007    5.0e-7 vs 2.4e-4 (474 x) / 3.9e-7 vs 1.8e-4 (474 x)
        (1000, 1280, 320)   0.005 / 0.006    6.9e-7 vs 2.2e-4 (317 x) / 5.7e-7 vs 1.8e-4 (312 x)
    test_linear_gelu_x3: fraction of the four-term bound, max |hi + lo - gelu| (reached beyond the clamp, 1.4e-6 |x|):
        (256, 256, 192)     0.085   1.6e-5      (300, 320, 192)   0.090   1.6e-5      (1000, 1280, 960)   0.019   2.4e-5
    The accumulation term is a worst-case bound and dominates the head-room; it also covers the 2^-25 absolute error of an
    fp16-subnormal `lo` (|value| < 0.06), which the 2^-21 |v| term alone would not.
    test_weight_images found the one defect: for bf16 sources hipcc had narrowed lo = fp16(w - hi) to the half subtraction
    hi - hi (+0 where the residue of a weight below fp16's normal range rounds to -0); convert2d_split_kernel now widens
    bf16 by its bits.
"""
import math

import pytest
import torch

from _ln_fold_ref import gelu64
from esm_amd import _native as nat
from esm_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT16 = 0x7BFF  # fp16 65504: no value below is ever rounded to it
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def sent_buf(rows, ld, dtype):
    """[rows, ld] of the sentinel: NaN for fp32, the bit pattern 0x7bff for the 16-bit types"""
    if dtype == torch.float32:
        return torch.full((rows, ld), float("nan"), device="cuda")
    return torch.full((rows, ld), SENT16, dtype=torch.int16, device="cuda").view(dtype)


def untouched(t):
    """every element of t still holds the sentinel"""
    if t.dtype == torch.float32:
        return bool(torch.isnan(t).all())
    return bool((t.contiguous().view(torch.int16) == SENT16).all())


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- gemm32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,pa,pc", [
    (1, 33, 32, 0, 0),         # every row clamp; one live column in the second MFMA
    (129, 33, 96, 4, 3),       # a second row tile with one row; both strides
    (128, 64, 32, 0, 0),       # exactly one full tile
    (200, 65, 320, 0, 0),      # a third column tile with one column
    (300, 1280, 1280, 0, 0),   # the dense head shape
])
def test_linear_f32(M, N, K, pa, pc):
    g = gen(11)
    lda, ldc = K + pa, N + pc
    a = torch.randn(M, lda, device="cuda", generator=g)  # columns >= K are finite and must not be read
    w = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    bias_t = torch.randn(N, device="cuda", generator=g)
    a64, w64 = a[:, :K].double(), w.double()
    for bias in (bias_t, None):
        b64 = bias.double() if bias is not None else torch.zeros(N, dtype=torch.float64, device="cuda")
        ref = a64 @ w64.t() + b64
        bound = (K + 2) * U * (a64.abs() @ w64.abs().t() + b64.abs())
        outs = {}
        for gelu in (0, 1):
            out = sent_buf(M + 1, ldc, torch.float32)
            ops.linear_f32(a, w, bias, gelu=gelu, out=out, M=M)
            assert untouched(out[M:]) and untouched(out[:M, N:]), "store outside the [M,N] footprint"
            assert not torch.isnan(out[:M, :N]).any(), "unwritten output element"
            outs[gelu] = out[:M, :N]
        pre = outs[0]
        r0 = ((pre.double() - ref).abs() / bound).max().item()
        # device erff: torch's fp32 gelu against the same function in fp64 on the fp32 pre-activations — two references,
        # neither is the kernel — in units of u max(1, |x|); the kernel may use 4x that
        unit = U * pre.double().abs().clamp(min=1.0)
        erf_meas = ((torch.nn.functional.gelu(pre).double() - gelu64(pre.double())).abs() / unit).max().item()
        allow = 4 * erf_meas * unit
        e1 = (outs[1].double() - gelu64(ref)).abs()
        r1 = (e1 / (1.13 * bound + allow)).max().item()
        # the two instantiations share the MFMA sequence: GELU of the plain run's fp32 output, within the erff allowance
        r2 = ((outs[1].double() - gelu64(pre.double())).abs() / allow).max().item()
        print(f"\nlinear_f32 ({M},{N},{K}) bias={bias is not None}: plain {r0:.3f} of the bound, erff measured "
              f"{erf_meas:.2f} u, gelu {r1:.3f} of its bound, gelu(plain run) {r2:.3f} of the allowance")
        assert r0 <= 1.0, r0
        assert erf_meas > 0 and r1 <= 1.0 and r2 <= 1.0, (erf_meas, r1, r2)


# ---- weight images -------------------------------------------------------------------------------------------------------
def spread(i, d):
    """where index i = head * d + dim goes when heads of d dims are spread over 64 slots (d = 128: the q / k slice order)"""
    h, j = divmod(i, d)
    if d == 128:  # slots hold the dims [0,32) | [64,96) | [32,64) | [96,128)
        order = list(range(0, 32)) + list(range(64, 96)) + list(range(32, 64)) + list(range(96, 128))
        return 128 * h + order.index(j)
    return 64 * h + (j if j < d // 2 else 32 + j - d // 2)  # first half at slot j, second half from slot 32


def planted(rows, cols, dtype, seed):
    """random weights with the values of interest among them, in the source dtype (on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows * cols, generator=g) * 0.05
    special = [0.0, 0.5, -0.25, 3.0, 1e-6, -1.3e-6, 3.1e-6, 6.2e-5, -7.123, -1e-3, 60000.0, -60000.0, 60010.3, 2.0 ** -24]
    pos = torch.linspace(0, rows * cols - 1, len(special)).long()
    assert len(set(pos.tolist())) == len(special)
    w[pos] = torch.tensor(special)
    return w.view(rows, cols).to(dtype)


IMAGE_CASES = [  # rows, cols, dst_ld, row_map, col_map, d
    (96, 128, 128, 0, 0, 64), (8, 64, 192, 0, 0, 64),
    (48, 128, 128, 1, 0, 16), (72, 128, 128, 1, 0, 24), (96, 128, 128, 1, 0, 32), (72, 128, 256, 1, 0, 24),
    (5, 48, 192, 0, 1, 16), (5, 72, 192, 0, 1, 24), (5, 96, 192, 0, 1, 32), (5, 72, 256, 0, 1, 24),
    (256, 64, 64, 1, 0, 128),
    (48, 48, 192, 1, 1, 16),  # both maps at once
]


@pytest.mark.parametrize("rows,cols,dst_ld,row_map,col_map,d", IMAGE_CASES)
def test_weight_images(rows, cols, dst_ld, row_map, col_map, d):
    rmap = torch.tensor([spread(r, d) if row_map else r for r in range(rows)])
    cmap = torch.tensor([spread(c, d) if col_map else c for c in range(cols)])
    dst_rows = (rows // d * (128 if d == 128 else 64)) if row_map else rows
    assert int(rmap.max()) < dst_rows and int(cmap.max()) < dst_ld
    for si, sdt in enumerate((torch.float32, torch.float16, torch.bfloat16)):
        src = planted(rows, cols, sdt, 20 + si)
        w32 = src.float()
        hi = w32.half()
        lo = (w32 - hi.float()).half()  # the subtraction is exact in fp32
        assert bool((lo[w32 == 0.5] == 0).all()) and bool(((hi != 0) & (hi.float().abs() < 6.1e-5)).any()) and bool((w32 < 0).any())
        src_dev = src.cuda()
        for parts, ddt in ((1, torch.float16), (1, torch.bfloat16), (1, torch.float32), (2, torch.float16), (3, torch.float16)):
            slots = {1: [w32.to(ddt)], 2: [hi, lo], 3: [hi, lo, hi]}[parts]
            want = sent_buf(dst_rows + 1, parts * dst_ld, ddt).cpu()
            for s, val in enumerate(slots):
                col = (cmap // 64) * (64 * parts) + 64 * s + cmap % 64
                want[rmap[:, None], col[None, :]] = val
            got = sent_buf(dst_rows + 1, parts * dst_ld, ddt)
            ops.split_weight_ex(src_dev, got, dst_ld, parts, row_map, col_map, d)
            got = got.cpu()
            same = bits(got) == bits(want)  # contents bit-equal, everything else still the sentinel
            assert bool(same.all()), (str(sdt), parts, str(ddt), same.logical_not().nonzero()[:8].tolist())
            if parts == 3:  # third slot == first, seen directly
                t = got[:dst_rows].view(dst_rows, dst_ld // 64, 3, 64)
                assert torch.equal(bits(t[:, :, 2]), bits(t[:, :, 0]))
            if parts == 2 and not row_map and not col_map:  # the f16x2 image of esmk_op_split_weight
                old = ops.split_weight(src_dev).cpu().view(rows, cols // 64, 2, 64)
                assert torch.equal(bits(got[:rows].view(rows, dst_ld // 64, 2, 64)[:, :cols // 64]), bits(old))


# ---- LayerNorm forms -----------------------------------------------------------------------------------------------------
LN_TOL = 2e-5  # the fp32 tolerance of tests/test_kernels_gpu.py::test_layernorm, on inputs of the same distribution


def ln_inputs(rows, E, seed):
    g = gen(seed)
    x = torch.randn(rows, E, device="cuda", generator=g) * 3 + 0.5
    gamma = 1 + 0.1 * torch.randn(E, device="cuda", generator=g)
    beta = 0.1 * torch.randn(E, device="cuda", generator=g)
    return x, gamma, beta


def ln64(x, gamma, beta, eps):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


@pytest.mark.parametrize("rows", [1, 7, 9])
@pytest.mark.parametrize("E", [64, 320, 1280, 2560])
def test_layernorm_x3(E, rows):
    x, gamma, beta = ln_inputs(rows, E, 31)
    ref = ln64(x, gamma, beta, 1e-5)
    worst = 0.0
    for variant in (None, 0):
        plain, _ = ops.layernorm(x, gamma, beta, torch.float16, variant=variant)
        for ldy in (3 * E, 3 * E + 64):
            y = sent_buf(rows + 1, ldy, torch.float16)
            y32 = sent_buf(rows + 1, E, torch.float32)
            ops.layernorm_ex(x, gamma, beta, y, y32, x3=True, variant=variant)
            assert untouched(y[rows:]) and untouched(y[:rows, 3 * E:]) and untouched(y32[rows:]), (variant, ldy)
            o = y32[:rows]
            err = (o.double() - ref).abs().max().item()
            worst = max(worst, err)
            assert err < LN_TOL, (variant, ldy, err)
            t = y[:rows, :3 * E].reshape(rows, E // 64, 3, 64)
            hi, hi2, lo = (t[:, :, s].reshape(rows, E) for s in range(3))
            assert torch.equal(bits(hi), bits(o.half())), (variant, ldy)
            assert torch.equal(bits(lo), bits((o - hi.float()).half())), (variant, ldy)
            assert torch.equal(bits(hi2), bits(hi)), (variant, ldy)
            assert torch.equal(bits(hi), bits(plain)), (variant, ldy)
            assert bool((lo != 0).any())
    print(f"\nlayernorm x3 E={E} rows={rows}: y32 max error {worst:.2e} (tolerance {LN_TOL:.0e})")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_layernorm_row_keep_and_row_map(dt):
    B, R, C, E = 2, 3, 5, 320
    rows = B * R * C
    x, gamma, beta = ln_inputs(rows, E, 32)
    keep = (torch.arange(rows, device="cuda") % 4 != 1).float()  # zeros and ones in every (b, r) row of the MSA
    assert 0 < keep.sum().item() < rows
    ref = ln64(x, gamma, beta, 1e-5)
    worst = 0.0
    for use_keep, use_map in ((True, True), (True, False), (False, True)):
        want = ref * keep.double()[:, None] if use_keep else ref
        if use_map:  # input rows (b,r,c) -> output rows (b,c,r)
            want = want.view(B, R, C, E).transpose(1, 2).reshape(rows, E)
        for variant in (None, 0):
            for ldy in (E, E + 64):
                y = sent_buf(rows + 1, ldy, dt)
                y32 = sent_buf(rows + 1, E, torch.float32)
                ops.layernorm_ex(x, gamma, beta, y, y32, operand_dtype=dt, row_keep=keep if use_keep else None,
                                 map_R=R if use_map else 0, map_C=C if use_map else 0, variant=variant)
                assert untouched(y[rows:]) and untouched(y[:rows, E:]) and untouched(y32[rows:]), (use_keep, use_map, variant, ldy)
                err = (y32[:rows].double() - want).abs().max().item()
                worst = max(worst, err)
                assert err < LN_TOL, (use_keep, use_map, variant, ldy, err)
                assert torch.equal(bits(y[:rows, :E]), bits(y32[:rows].to(dt))), (use_keep, use_map, variant, ldy)
    print(f"\nlayernorm row_keep / row map {dt}: y32 max error {worst:.2e} (tolerance {LN_TOL:.0e})")


def test_layernorm_eps():
    """Rows of spread 1e-4 around 0 (variance ~1e-8; centred, so that the fp32 mean does not cost the digits the
    tolerance is about): eps = 1e-12 (ESM-1) normalises them to unit scale, eps = 1e-5 leaves them at ~0.03."""
    rows, E = 7, 320
    _, gamma, beta = ln_inputs(rows, E, 33)
    x = 1e-4 * torch.randn(rows, E, device="cuda", generator=gen(34))
    out = {}
    for eps in (1e-12, 1e-5):
        for variant in (None, 0):
            y32 = sent_buf(rows + 1, E, torch.float32)
            ops.layernorm_ex(x, gamma, beta, None, y32, eps=eps, variant=variant)
            assert untouched(y32[rows:])
            err = (y32[:rows].double() - ln64(x, gamma, beta, eps)).abs().max().item()
            print(f"\nlayernorm eps={eps:g} variant={variant}: max error {err:.2e} (tolerance {LN_TOL:.0e})")
            assert err < LN_TOL, (eps, variant, err)
            out[eps] = y32[:rows]
    ratio = (out[1e-12] - beta).norm(dim=1) / (out[1e-5] - beta).norm(dim=1)  # sqrt((1e-8 + 1e-5) / 1e-8) ~ 31.6
    print(f"layernorm eps: |y(1e-12) - beta| / |y(1e-5) - beta| per row {ratio.min().item():.1f} .. {ratio.max().item():.1f}")
    assert ratio.min().item() > 10


# ---- the f16x3 operands, shared by the two GEMM tests ---------------------------------------------------------------------
def x3_operands(M, N, K, seed):
    """A3 [M+1, 3K] hi | hi | lo from the LayerNorm entry (gamma = 1, beta = 0, pre-normalised rows: a pure split of the
    fp32 rows A32 it also returns), W3 [N+1, 3K] hi | lo | hi from the weight-image entry; the spare rows hold the sentinel."""
    g = gen(seed)
    x = torch.nn.functional.layer_norm(torch.randn(M, K, device="cuda", generator=g), (K,))
    one, zero = torch.ones(K, device="cuda"), torch.zeros(K, device="cuda")
    a3 = sent_buf(M + 1, 3 * K, torch.float16)
    a32 = sent_buf(M + 1, K, torch.float32)
    ops.layernorm_ex(x, one, zero, a3, a32, x3=True)
    w = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    w3 = sent_buf(N + 1, 3 * K, torch.float16)
    ops.split_weight_ex(w, w3, K, 3)
    assert untouched(a3[M:]) and untouched(a32[M:]) and untouched(w3[N:])
    return a3[:M], a32[:M], w3[:N], w


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 264, 192), (1000, 1280, 320)])
def test_f16x3_product(M, N, K):
    a3, a32, w3, w = x3_operands(M, N, K, 41)
    g = gen(42)
    bias = torch.randn(N, device="cuda", generator=g)
    resid = torch.randn(M, N, device="cuda", generator=g)
    a3d, w3d = a3.double(), w3.double()
    three = a3d @ w3d.t() + bias.double()  # A_hi W_hi + A_hi W_lo + A_lo W_hi, the sum the mode specifies
    mag = a3d.abs() @ w3d.abs().t() + bias.double().abs()
    full = a32.double() @ w.double().t() + bias.double()  # the unrounded operands
    a16, w16 = a32.half(), w.half()
    try:
        for epi in (nat.EPI_STORE_F32, nat.EPI_RESID_F32):
            r64 = resid.double() if epi == nat.EPI_RESID_F32 else 0.0
            bound = (3 * K + 2) * U * (mag + (resid.double().abs() if epi == nat.EPI_RESID_F32 else 0.0))
            got = {}
            for impl in (0, 8, 9):
                nat.check(nat.lib.esmk_debug_gemm_impl(impl, 0))
                buf = sent_buf(M + 1, N, torch.float32)
                if epi == nat.EPI_RESID_F32:
                    buf[:M] = resid
                ops.linear(a3, w3, bias, epi, out=buf[:M])
                assert untouched(buf[M:]) and not torch.isnan(buf[:M]).any(), (epi, impl)
                got[impl] = buf[:M]
            assert torch.equal(got[8], got[9]) and torch.equal(got[0], got[9]), epi
            nat.check(nat.lib.esmk_debug_gemm_impl(0, 0))
            pbuf = resid.clone() if epi == nat.EPI_RESID_F32 else None
            plain = ops.linear(a16, w16, bias, epi, out=pbuf)
            r = ((got[0].double() - (three + r64)).abs() / bound).max().item()
            scale = (full + r64).abs().max().item()
            e3 = (got[0].double() - (full + r64)).abs().max().item() / scale
            ep = (plain.double() - (full + r64)).abs().max().item() / scale
            print(f"\nf16x3 product ({M},{N},{K}) epi {epi}: {r:.3f} of the accumulation bound; against the unrounded "
                  f"operands x3 {e3:.2e}, plain fp16 {ep:.2e}, ratio {ep / e3:.0f}")
            assert r <= 1.0, (epi, r)
            assert ep >= 8 * e3, (epi, e3, ep)
    finally:
        nat.lib.esmk_debug_gemm_impl(0, 0)


def gelu_x3_bound(a3d, w3d, bias, pre, v, K):
    """the four-term bound of hi + lo = v against gelu64(pre): accumulation, the polynomial, the split"""
    acc = (3 * K + 2) * U * (a3d.abs() @ w3d.abs().t() + bias.double().abs())
    poly = 1.4e-6 * pre.abs().clamp(min=1.0).where(pre.abs() > 4.75, torch.ones_like(pre))  # common.h, the degree-11 set
    return 1.13 * acc + poly + 2.0 ** -21 * v.abs()


@pytest.mark.parametrize("M,N,K3", [(256, 256, 192), (300, 320, 192), (1000, 1280, 960)])
def test_linear_gelu_x3(M, N, K3):
    K = K3 // 3
    a3, _, w3, _ = x3_operands(M, N, K, 51)
    g = gen(52)
    # pre-activations a . w ~ N(0,1) shifted by a bias that sweeps +-8: both clamp branches (|x| > 4.75) are taken
    bias = (torch.linspace(-8, 8, N, device="cuda") + 0.3 * torch.randn(N, device="cuda", generator=g))[torch.randperm(N, device="cuda", generator=g)]
    a3d, w3d = a3.double(), w3.double()
    pre = a3d @ w3d.t() + bias.double()
    assert bool((pre > 4.75).any()) and bool((pre < -4.75).any()) and bool((pre.abs() < 1).any())
    want = gelu64(pre)
    out3 = sent_buf(M + 1, 3 * N, torch.float16)
    ops.linear_gelu_x3(a3, w3, bias, out3, M=M)
    assert untouched(out3[M:]), "store behind the last row"
    assert not (bits(out3[:M]) == SENT16).any(), "unwritten output element"
    t = out3[:M].view(M, N // 64, 3, 64)
    hi, hi2, lo = (t[:, :, s].reshape(M, N) for s in range(3))
    assert torch.equal(bits(hi2), bits(hi))
    v = hi.double() + lo.double()
    bound = gelu_x3_bound(a3d, w3d, bias, pre, v, K)
    r = ((v - want).abs() / bound).max().item()
    rem = (lo.double().abs() - (2.0 ** -11 * hi.double().abs() + U)).max().item()
    print(f"\nlinear_gelu_x3 ({M},{N},{K3}): {r:.3f} of the bound, max |hi + lo - gelu| {(v - want).abs().max().item():.2e}, "
          f"pre in [{pre.min().item():.1f}, {pre.max().item():.1f}]")
    assert r <= 1.0, r
    assert rem <= 0, rem  # lo is a genuine remainder of hi
    assert bool((lo != 0).any())
