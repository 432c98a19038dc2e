"""The LayerNorm-fold ops (reference esm/modules.py:120-140) one launch at a time at their EDGES, in fp16
and bf16, against the fp64 reference and the a-priori bounds of tests/_ln_fold_ref.py: rowstats_kernel, fold_weight_kernel
(with the head spread of head_dim 16 / 24 / 32), gemm9's LNF producer and GELU consumer at both tile heights,
ln_finalize_kernel, a four-step producer -> finalize chain, and the cancellation of a per-row constant against the centred
image on the device.  tests/test_ln_fold_gpu.py checks the same ops at model shapes in fp16 and the chain end to end; what
it cannot see is here: one row, one row past a wave block (64 / 128) and past a tile (256), an 8-column slab, bf16, rows
whose mean lags or that are constant, and stray stores.

Every output carries guard rows (and guard columns where it has a row stride) holding a sentinel — 7.0 for operand-dtype
and fp32 data, NaN for ln_part — and ln_rstd / ln_mean are padded with NaN to the next multiple of 256 rows: the guards
must be unchanged and every valid output finite.  Every GEMM case asserts its plan (esmk_debug_gemm_plan, flag 4).

Every test prints its error as a fraction of the bound (`pytest -s`).  MEASURED on an MI355X, largest fraction over the
cases of a test, fp16 / bf16:
    test_rowstats            mean 0.12, rstd 0.22 of the two-pass bound (both dtypes: the statistics are fp32)
    test_fold_weight         image 0.997 / 0.999 (half an ulp is reached by a round-to-nearest store), bias2 0.011
    test_producer            out 0.025, S1 0.013 / 0.014, S2 0.031; out and h16 bit-equal in all 20 cases
    test_ln_finalize_alone   mean 0.12, rstd 0.32 (the CPU emulation of the documented order: 0.12, 0.32)
    test_chain_does_not_drift  steps 0 - 3: mean 0.037 0.045 0.037 0.037 / 0.037 0.053 0.045 0.047,
                             rstd 0.155 0.184 0.152 0.152 / 0.126 0.143 0.166 0.196 of each step's own bound
    test_consumer            0.986 / 0.998 (the half ulp); 77 k values on the left tail and 77 k beyond the clamp on the right
    test_constant_cancels_on_the_device  0.42 / 0.36 of the allowance, the row-sum term at most 0.08 / 0.10 of it;
                             max |rowsum(W'')| of the image the kernel wrote 5.4e-4 / 5.0e-3
No kernel defect was found.
"""
import ctypes
import math

import pytest
import torch

import _ln_fold_ref as R
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
G = 2  # guard rows
SENT = 7.0
NAN = float("nan")


def full(shape, fill, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def is_sent(t):
    return bool((t == SENT).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def pad256(v, fill=NAN):
    """fp32 [M] -> [M rounded up to 256], the pad holding NaN: a pad value that reaches a valid row shows"""
    out = full(((v.numel() + 255) // 256 * 256,), fill)
    out[: v.numel()] = v
    return out


def frac(err, bound):
    return (err / bound).max().item()


def assert_plan(M, Nn, K, epi):
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, Nn, K, epi, 4, out))
    assert out[0] == 9, (M, Nn, K, epi, out[0])


def linear_ln(a, w, bias, bias2, out, epilogue, M, rstd=None, h16=None, part=None, parts=0, mean=None, half_m=0):
    Nn, K = w.shape
    assert_plan(M, Nn, K, epilogue)
    N.check(N.lib.esmk_op_linear_ln(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(bias2), N.ptr(out), M, Nn, K, epilogue,
                                    R.DT_CODE[a.dtype], N.ptr(rstd), N.ptr(h16), h16.shape[1] if h16 is not None else 0,
                                    N.ptr(part), parts, N.ptr(mean), half_m, N.cur_stream()))


def run_producer(a, w, bias, x, mean_pad, half_m, spare_slab=1):
    """x fp32 [M + G, N] (guard rows SENT) is updated in place; returns (h16 [M + G, ldh], part [M + G, P + spare, 2])"""
    M, (Nn, K) = a.shape[0], w.shape
    P = (Nn + 127) // 128
    h16 = full((M + G, (Nn + 63) // 64 * 64 + 64), SENT, a.dtype)
    part = full((M + G, P + spare_slab, 2), NAN)
    linear_ln(a, w, bias, None, x, N.EPI_RESID_F32, M, h16=h16, part=part, parts=P + spare_slab, mean=mean_pad, half_m=half_m)
    return h16, part


# ---- rowstats -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("E", R.ROWSTATS_E)  # both sides of every NCH bucket (512, 1280, 2560) and the largest
@pytest.mark.parametrize("rows", R.ROWSTATS_ROWS)  # one row (a wave's second row is a clamped copy); 9: a second block with one row
def test_rowstats(rows, E, pad, dtype):
    x = R.make_rows(rows, E, seed=E + rows).cuda()
    ldy = E + pad
    y = full((rows + G, ldy), SENT, dtype)
    mean, rstd = full((rows + G,), SENT), full((rows + G,), SENT)
    N.check(N.lib.esmk_op_rowstats(N.ptr(x), N.ptr(y), N.ptr(mean), N.ptr(rstd), rows, E, ldy, R.DT_CODE[dtype], N.cur_stream()))
    assert is_sent(y[rows:]) and is_sent(y[:rows, E:]) and is_sent(mean[rows:]) and is_sent(rstd[rows:]), "stray store"
    assert torch.isfinite(y[:rows, :E].float()).all() and torch.isfinite(mean[:rows]).all() and torch.isfinite(rstd[:rows]).all()
    assert torch.equal(y[:rows, :E], (x - mean[:rows, None]).to(dtype))  # the kernel's own mean, subtracted in fp32, one rounding
    m64, _, r64 = R.ln_stats(x)
    b_mean, b_rstd = R.rowstats_bounds(x)
    f_mean = frac((mean[:rows].double() - m64).abs(), b_mean)
    f_rstd = frac((rstd[:rows].double() - r64).abs() / r64, b_rstd)
    print(f"\nrowstats rows={rows} E={E} ldy={ldy} {dtype}: mean {f_mean:.3f}, rstd {f_rstd:.3f} of the two-pass bound")
    assert f_mean <= 1.0 and f_rstd <= 1.0, (f_mean, f_rstd)


# ---- fold_weight ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("wdt", [torch.float32, torch.float16, torch.bfloat16], ids=["w32", "w16", "wbf"])
@pytest.mark.parametrize("d", [64, 16, 24, 32])
@pytest.mark.parametrize("Nn,K,ld", [(8, 64, 64), (96, 480, 512), (130, 1280, 1280)])
def test_fold_weight(Nn, K, ld, d, wdt, dtype):
    """head_dim 64 runs the entry without head_dim (any N); below 64 N is rounded up to whole heads and the image has
    N / d * 64 rows, of which the slots no row maps to must keep the sentinel."""
    if d < 64:
        Nn = (Nn + d - 1) // d * d
    g = torch.Generator().manual_seed(Nn + K + d)
    w = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).to(wdt)
    w[1] = 0
    gamma = 1 + 0.1 * torch.randn(K, generator=g)
    gamma[0], gamma[1] = 0.0, 1e-4
    beta = 0.1 * torch.randn(K, generator=g)
    w, gamma, beta = w.cuda(), gamma.cuda(), beta.cuda()
    rows_out = Nn if d == 64 else Nn // d * 64
    dst = full((rows_out + G, ld), SENT, dtype)
    b2 = full((rows_out + G,), SENT)
    if d == 64:
        N.check(N.lib.esmk_op_fold_weight(N.ptr(w), R.DT_CODE[wdt], N.ptr(gamma), N.ptr(beta), N.ptr(dst), R.DT_CODE[dtype],
                                          N.ptr(b2), Nn, K, ld, N.cur_stream()))
    else:
        N.check(N.lib.esmk_op_fold_weight_ex(N.ptr(w), R.DT_CODE[wdt], N.ptr(gamma), N.ptr(beta), N.ptr(dst), R.DT_CODE[dtype],
                                             N.ptr(b2), Nn, K, ld, d, N.cur_stream()))
    f = R.fold_image(w, gamma, beta, dtype, d)
    rows = f["rows"]
    hole = torch.ones(rows_out + G, dtype=torch.bool, device="cuda")
    hole[rows] = False
    assert int(hole.sum()) == rows_out + G - Nn
    assert is_sent(dst[hole]) and is_sent(b2[hole]) and is_sent(dst[:, K:]), "store outside the mapped rows / past K"
    got = dst[rows, :K].double()
    assert torch.isfinite(got).all() and torch.isfinite(b2[rows]).all()
    f_img = frac((got - f["exact"]).abs(), f["image_bound"])
    f_b2 = frac((b2[rows].double() - f["bias2"]).abs(), f["bias2_bound"].clamp_min(1e-30))
    print(f"\nfold_weight ({Nn},{K},{ld}) d={d} {wdt}->{dtype}: image {f_img:.3f}, bias2 {f_b2:.3f} of the bound")
    assert f_img <= 1.0 and f_b2 <= 1.0, (f_img, f_b2)
    assert not got[1].any() and b2[rows[1]].item() == 0.0  # the all-zero weight row
    if d == 64 and Nn >= 64:  # head_dim 64 through the entry with head_dim: the same bits on the whole heads
        n64 = Nn // 64 * 64
        dst2, b22 = full((n64 + G, ld), SENT, dtype), full((n64 + G,), SENT)
        N.check(N.lib.esmk_op_fold_weight_ex(N.ptr(w), R.DT_CODE[wdt], N.ptr(gamma), N.ptr(beta), N.ptr(dst2), R.DT_CODE[dtype],
                                             N.ptr(b22), n64, K, ld, 64, N.cur_stream()))
        assert torch.equal(dst2[:n64], dst[:n64]) and torch.equal(b22[:n64], b2[:n64]) and is_sent(dst2[n64:]) and is_sent(b22[n64:])


# ---- producer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("half_m", [1, -1])
@pytest.mark.parametrize("M,Nn,K", R.PRODUCER_SHAPES)
def test_producer(M, Nn, K, half_m, dtype):
    """a single row; an 8-column slab; one row past the wave block and past the tile; FULL and clipped blocks in one launch;
    whole tiles only.  Rows of all four classes with mean_prev lagging by 0 / 0.01 / 1 / 10 spreads in one launch."""
    a, w, bias, x0, mean_prev = (t.cuda() for t in R.producer_case(M, Nn, K, dtype, seed=100 + M))
    plain = ops.linear(a, w, bias, N.EPI_RESID_F32, out=x0.clone(), half_m=half_m)
    x = full((M + G, Nn), SENT)
    x[:M] = x0
    h16, part = run_producer(a, w, bias, x, pad256(mean_prev), half_m)
    P = (Nn + 127) // 128
    out = x[:M]
    assert is_sent(x[M:]) and is_sent(h16[M:]) and is_sent(h16[:M, Nn:]), "stray store"
    assert all_nan(part[M:]) and all_nan(part[:M, P:]), "stray partial sums"
    assert torch.isfinite(out).all() and torch.isfinite(part[:M, :P]).all() and torch.isfinite(h16[:M, :Nn].float()).all()
    assert torch.equal(out, plain)  # bit-equal to the plain residual epilogue of the same tile height
    ref, bound = R.producer(a, w, bias, x0)
    f_out = frac((out.double() - ref).abs(), bound)
    d, h_ref, p_ref, p_bound = R.producer_side(out, mean_prev, dtype)
    assert torch.equal(h16[:M, :Nn], h_ref)
    err = (part[:M, :P].double() - p_ref).abs()
    ok = err <= p_bound
    f_s1 = frac(err[..., 0], p_bound[..., 0].clamp_min(1e-30))
    f_s2 = frac(err[..., 1], p_bound[..., 1].clamp_min(1e-30))
    print(f"\nproducer ({M},{Nn},{K}) half_m={half_m} {dtype}: out {f_out:.3f}, S1 {f_s1:.3f}, S2 {f_s2:.3f} of the bound")
    assert f_out <= 1.0 and bool(ok.all()), (f_out, f_s1, f_s2)


# ---- ln_finalize alone ------------------------------------------------------------------------------------------------------
def check_finalize(mean, rstd, x, mean_prev, what):
    """kernel mean / rstd [rows] against the fp64 statistics of the fp32 rows x, inside the finalize bounds"""
    m64, v64, r64 = R.ln_stats(x)
    b_mean, b_rstd = R.finalize_bounds(x, mean_prev)
    assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    f_mean = frac((mean.double() - m64).abs(), b_mean)
    f_rstd = frac((rstd.double() - r64).abs() / r64, b_rstd)
    print(f"\n{what}: mean {f_mean:.3f}, rstd {f_rstd:.3f} of the finalize bound")
    assert f_mean <= 1.0 and f_rstd <= 1.0, (what, f_mean, f_rstd)
    const = v64 == 0
    if const.any():
        # exactly constant rows, any lag: the clamp at 0 holds and the cancellation S2 / E - dm^2 stays below 1e-3 of eps.
        # The upper end is eps^-1/2 as fp32 computes it: 1e-5f, the root and the division round once each (4 * 2^-23).
        top = R.EPS ** -0.5
        r = rstd[const].double()
        assert (r >= (1 - 1e-3) * top).all() and (r <= (1 + 4 * 2.0 ** -23) * top).all(), (r.min().item(), r.max().item())
    return f_mean, f_rstd


@pytest.mark.parametrize("rows", R.FINALIZE_ROWS)
@pytest.mark.parametrize("parts", R.FINALIZE_PARTS)
def test_ln_finalize_alone(parts, rows):
    """Partial sums built in fp64 from rows of the four classes and rounded to fp32 (the kernel has no operand dtype: one
    instantiation).  300 rows: a second workgroup."""
    x, mean_prev = (t.cuda() for t in R.finalize_case(rows, parts))
    E = x.shape[1]
    _, _, p64, _ = R.producer_side(x, mean_prev, torch.float16)
    part = full((rows + G, parts, 2), NAN)
    part[:rows] = p64.float()
    before = part.clone()
    mean, rstd = full((rows + G,), SENT), full((rows + G,), SENT)
    mean[:rows] = mean_prev
    N.check(N.lib.esmk_op_ln_finalize(N.ptr(part), N.ptr(mean), N.ptr(rstd), rows, parts, E, N.cur_stream()))
    assert is_sent(mean[rows:]) and is_sent(rstd[rows:]) and torch.equal(part.view(torch.int32), before.view(torch.int32))
    check_finalize(mean[:rows], rstd[:rows], x, mean_prev, f"ln_finalize rows={rows} parts={parts}")


# ---- chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_chain_does_not_drift(dtype):
    """rowstats, then four producer -> finalize steps, each producer reading the mean the previous finalize wrote: after
    every step mean and rstd are within the finalize bound OF THAT STEP of the fp64 statistics of the kernel's own rows."""
    c = R.CHAIN
    M, E = c["M"], c["E"]
    P = (E + 127) // 128
    x = full((M + G, E), SENT)
    x[:M] = R.make_rows(M, E, seed=31).cuda()
    y = full((M, E), SENT, dtype)
    mean, rstd = full((256,), NAN), full((256,), NAN)
    N.check(N.lib.esmk_op_rowstats(N.ptr(x), N.ptr(y), N.ptr(mean), N.ptr(rstd), M, E, E, R.DT_CODE[dtype], N.cur_stream()))
    b_mean, b_rstd = R.rowstats_bounds(x[:M])
    m64, _, r64 = R.ln_stats(x[:M])
    assert frac((mean[:M].double() - m64).abs(), b_mean) <= 1.0 and frac((rstd[:M].double() - r64).abs() / r64, b_rstd) <= 1.0
    for step in range(c["steps"]):
        a, w, bias, _, _ = (t.cuda() for t in R.producer_case(M, E, c["K"], dtype, seed=40 + step))
        mean_before = mean[:M].clone()
        h16, part = run_producer(a, w, bias, x, mean, half_m=0, spare_slab=0)
        assert torch.equal(h16[:M, :E], (x[:M] - mean_before[:, None]).to(dtype))
        N.check(N.lib.esmk_op_ln_finalize(N.ptr(part), N.ptr(mean), N.ptr(rstd), M, P, E, N.cur_stream()))
        assert is_sent(x[M:]) and all_nan(mean[M:]) and all_nan(rstd[M:]) and all_nan(part[M:])
        check_finalize(mean[:M], rstd[:M], x[:M], mean_before, f"chain {dtype} step {step}")


# ---- consumer ---------------------------------------------------------------------------------------------------------------
def run_consumer(a, w, bias, bias2, rstd, half_m):
    """out [M, N] of the GELU consumer; guard rows checked here (the output has no row stride: no guard columns)"""
    M, Nn = a.shape[0], w.shape[0]
    out = full((M + G, Nn), SENT, a.dtype)
    linear_ln(a, w, bias, bias2, out, N.EPI_GELU_T, M, rstd=pad256(rstd), half_m=half_m)
    assert is_sent(out[M:]), "stray store"
    assert torch.isfinite(out[:M].float()).all()
    return out[:M]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("half_m", [1, -1])
@pytest.mark.parametrize("M,Nn,K", R.CONSUMER_SHAPES)
def test_consumer(M, Nn, K, half_m, dtype):
    """rstd log-uniform in [0.05, 300] per row (a constant row produces 316): most pre-activations of the large-rstd rows
    lie beyond the polynomial's clamp, on both tails."""
    g = torch.Generator().manual_seed(200 + M)
    a = torch.randn(M, K, generator=g).to(dtype).cuda()
    w = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).to(dtype).cuda()
    bias, bias2 = torch.randn(Nn, generator=g).cuda(), torch.randn(Nn, generator=g).cuda()
    rstd = (0.05 * (300 / 0.05) ** torch.rand(M, generator=g)).cuda()
    out = run_consumer(a, w, bias, bias2, rstd, half_m)
    pre, pre_bound = R.consumer(a, w, bias, bias2, rstd)
    val, bound = R.gelu_out_bound(pre, pre_bound, dtype)
    f = frac((out.double() - val).abs(), bound)
    tail = pre + pre_bound < -R.GELU_SETS[True][0]
    print(f"\nconsumer ({M},{Nn},{K}) half_m={half_m} {dtype}: {f:.3f} of the bound; {int(tail.sum())} values on the left tail, "
          f"{int((pre - pre_bound > 4).sum())} beyond the clamp on the right")
    assert f <= 1.0, f
    assert (out[tail] <= 0).all()  # the one-signed residue of the left tail


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_cancels_on_the_device(dtype):
    """The consumer on a = T(x - c), c = mean + delta sigma: against delta = 0 the outputs may move by what the constant
    meets in the row sums of the image THE KERNEL WROTE, |delta sigma| rstd |rowsum(W'')| (times max |gelu'|), by the
    rounding of the two a (half an ulp per element, through |W''|), the two accumulations, the polynomial at two points and
    half an output ulp each."""
    M, E, Nn = 66, 320, 136
    g = torch.Generator().manual_seed(9)
    x = R.make_rows(M, E, seed=77).cuda()
    w = (torch.randn(Nn, E, generator=g) / math.sqrt(E)).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(E, generator=g)).cuda(), (0.1 * torch.randn(E, generator=g)).cuda()
    bias = torch.randn(Nn, generator=g).cuda()
    img, b2 = full((Nn, E), SENT, dtype), full((Nn,), SENT)
    N.check(N.lib.esmk_op_fold_weight(N.ptr(w), 0, N.ptr(gamma), N.ptr(beta), N.ptr(img), R.DT_CODE[dtype], N.ptr(b2), Nn, E, E,
                                      N.cur_stream()))
    rowsum = img.double().sum(-1).abs()
    mean, var, rstd64 = R.ln_stats(x)
    sigma, rstd = var.sqrt(), rstd64.float()
    runs = {}
    for delta in (0.0, 0.5, -0.5):
        a = (x.double() - (mean + delta * sigma)[:, None]).to(dtype)
        pre, pre_bound = R.consumer(a, img, bias, b2, rstd)
        rounding = rstd.double()[:, None] * (R.half_ulp(a.double(), dtype) @ img.double().abs().T)
        runs[delta] = (run_consumer(a, img, bias, b2, rstd, half_m=0).double(), pre, pre_bound + rounding)
    out0, pre0, slack0 = runs[0.0]
    for delta in (0.5, -0.5):
        out, pre, slack = runs[delta]
        shift = (abs(delta) * sigma * rstd.double())[:, None] * rowsum[None, :]
        moved = R.GELU_SLOPE * (shift + slack + slack0)
        allow = moved + 2 * R.gelu_poly_bound(pre0, True, moved) + 2 * R.half_ulp(out0.abs() + moved, dtype)
        f = frac((out - out0).abs(), allow)
        f_shift = (R.GELU_SLOPE * shift / allow).max().item()
        print(f"\ncancellation {dtype} delta={delta}: {f:.3f} of the allowance (the row-sum term is at most {f_shift:.3f} of it); "
              f"max |rowsum(W'')| {rowsum.max().item():.2e}")
        assert f <= 1.0, (delta, f)
