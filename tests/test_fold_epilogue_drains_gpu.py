"""gemm9's LayerNorm-fold epilogues at the places where a wrong wait count or a wrong address would show ("fold
producer without scratch"): the residual producer (EPI_RESID_F32 + ln_part) addresses out, h16, ln_mean and ln_part as a scalar
base of the wave's block plus a 32-bit lane offset and waits for its residual pieces by count; the fc1 consumer (EPI_GELU_T +
ln_rstd) fetches bias, bias2 and the row scales while the next tile's LDS-DMA pieces are in flight.  A stale or misplaced value is
what either would produce, so the checks are bit comparisons between launches that must agree exactly (an output element depends
on its row of A, its row of W and its row / column vectors alone, and sees the same MFMA sequence in every tiling) on top of the
a-priori bounds of tests/_ln_fold_ref.py:

  * one full tile and its clipped twin: rows and columns present in both launches are bit-equal (consumer output; producer
    out, h16 and the ln_part slabs complete in both), every launch inside the bounds, guards untouched;
  * two tiles per workgroup (272 full tiles on 256 workgroups; K = 64 and 192: the next tile's LDS-DMA pieces are in flight
    during the epilogue, which the counted waits must get right): each 256-row slice is bit-equal to the slice launched alone;
  * producer statistics: ln_part bit-equal between the two tile heights and between full and clipped blocks; ln_mean is
    padded with NaN, which must not reach a valid row.

fp16 and bf16, both tile heights (half_m 1 / -1), bias2 given and absent.  The library has no STORE form of the fold consumer
(esmk_op_linear_ln takes epilogues 2 and 4), so the consumer is the GELU one.  Every launch asserts plan 9.
"""
import ctypes
import math

import pytest
import torch

import _ln_fold_ref as R
from esm_amd import _native as N

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
G = 2  # guard rows
SENT = 7.0
NAN = float("nan")

# (M, N) of the full launch first, then its clipped twins; one K per group (operands are slices of one set)
GROUPS = {64: [(256, 256), (255, 256), (257, 264)], 128: [(512, 512), (511, 504)]}


def full(shape, fill, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def is_sent(t):
    return bool((t == SENT).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def pad256(v):
    out = full(((v.numel() + 255) // 256 * 256,), NAN)
    out[: v.numel()] = v
    return out


def frac(err, bound):
    return (err / bound).max().item()


def linear_ln(a, w, bias, bias2, out, epilogue, M, rstd=None, h16=None, part=None, parts=0, mean=None, half_m=0):
    Nn, K = w.shape
    plan = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, Nn, K, epilogue, 4, plan))
    assert plan[0] == 9, (M, Nn, K, epilogue, plan[0])
    N.check(N.lib.esmk_op_linear_ln(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(bias2), N.ptr(out), M, Nn, K, epilogue,
                                    R.DT_CODE[a.dtype], N.ptr(rstd), N.ptr(h16), h16.shape[1] if h16 is not None else 0,
                                    N.ptr(part), parts, N.ptr(mean), half_m, N.cur_stream()))


def run_consumer(a, w, bias, bias2, rstd, half_m):
    """GELU consumer on contiguous operands; rstd is padded with NaN to whole tiles; returns out [M, N] (guard rows checked)"""
    M, Nn = a.shape[0], w.shape[0]
    out = full((M + G, Nn), SENT, a.dtype)
    linear_ln(a, w, bias, bias2, out, N.EPI_GELU_T, M, rstd=pad256(rstd), half_m=half_m)
    assert is_sent(out[M:]), "stray store"
    assert torch.isfinite(out[:M].float()).all()
    return out[:M]


def run_producer(a, w, bias, x0, mean, half_m):
    """producer on contiguous operands; ln_mean padded with NaN.  Returns (out [M, N], h16 [M, N], part [M, P, 2]); guard rows
    of all three, guard columns of h16 and the spare slab of ln_part checked."""
    M, (Nn, K) = a.shape[0], w.shape
    P = (Nn + 127) // 128
    x = full((M + G, Nn), SENT)
    x[:M] = x0
    h16 = full((M + G, (Nn + 63) // 64 * 64 + 64), SENT, a.dtype)
    part = full((M + G, P + 1, 2), NAN)
    linear_ln(a, w, bias, None, x, N.EPI_RESID_F32, M, h16=h16, part=part, parts=P + 1, mean=pad256(mean), half_m=half_m)
    assert is_sent(x[M:]) and is_sent(h16[M:]) and is_sent(h16[:M, Nn:]), "stray store"
    assert all_nan(part[M:]) and all_nan(part[:M, P:]), "stray partial sums"
    assert torch.isfinite(x[:M]).all() and torch.isfinite(part[:M, :P]).all() and torch.isfinite(h16[:M, :Nn].float()).all()
    return x[:M], h16[:M, :Nn], part[:M, :P]


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(x, y):
    return torch.equal(bits(x), bits(y))


# ---- one full tile and its clipped twins ------------------------------------------------------------------------------------
_consumer_cases = {}


def consumer_operands(K, dtype):
    """operands of the largest launch of the group (the others are slices) and the fp64 reference with its bound, once"""
    key = (K, dtype)
    if key not in _consumer_cases:
        Mx, Nx = max(m for m, _ in GROUPS[K]), max(n for _, n in GROUPS[K])
        g = torch.Generator().manual_seed(300 + K)
        a = torch.randn(Mx, K, generator=g).to(dtype).cuda()
        w = (torch.randn(Nx, K, generator=g) / math.sqrt(K)).to(dtype).cuda()
        bias, bias2 = torch.randn(Nx, generator=g).cuda(), torch.randn(Nx, generator=g).cuda()
        rstd = (0.05 * (300 / 0.05) ** torch.rand(Mx, generator=g)).cuda()
        refs = {}
        for with2 in (False, True):
            pre, pre_bound = R.consumer(a, w, bias, bias2 if with2 else None, rstd)
            refs[with2] = R.gelu_out_bound(pre, pre_bound, dtype)
        _consumer_cases[key] = (a, w, bias, bias2, rstd, refs)
    return _consumer_cases[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with2", [False, True], ids=["bias", "bias+bias2"])
@pytest.mark.parametrize("half_m", [1, -1])
@pytest.mark.parametrize("K", sorted(GROUPS))
def test_consumer_full_and_clipped(K, half_m, with2, dtype):
    a, w, bias, bias2, rstd, refs = consumer_operands(K, dtype)
    val, bound = refs[with2]
    outs = []
    for M, Nn in GROUPS[K]:
        out = run_consumer(a[:M].contiguous(), w[:Nn].contiguous(), bias[:Nn].contiguous(), bias2[:Nn].contiguous() if with2 else None,
                           rstd[:M], half_m)
        f = frac((out.double() - val[:M, :Nn]).abs(), bound[:M, :Nn])
        print(f"\nconsumer ({M},{Nn},{K}) half_m={half_m} bias2={with2} {dtype}: {f:.3f} of the bound")
        assert f <= 1.0, (M, Nn, f)
        outs.append(out)
    for (M, Nn), out in zip(GROUPS[K][1:], outs[1:]):
        m, n = min(M, GROUPS[K][0][0]), min(Nn, GROUPS[K][0][1])
        assert same_bits(out[:m, :n], outs[0][:m, :n]), f"full and clipped ({M},{Nn}) launches differ"


_producer_cases = {}


def producer_operands(K, dtype):
    key = (K, dtype)
    if key not in _producer_cases:
        Mx, Nx = max(m for m, _ in GROUPS[K]), max(n for _, n in GROUPS[K])
        a, w, bias, x0, mean_prev = (t.cuda() for t in R.producer_case(Mx, Nx, K, dtype, seed=400 + K))
        _producer_cases[key] = (a, w, bias, x0, mean_prev, R.producer(a, w, bias, x0))
    return _producer_cases[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", sorted(GROUPS))
def test_producer_full_and_clipped_and_both_heights(K, dtype):
    """out, h16 and ln_part: inside the bounds in every launch; bit-equal between the tile heights; bit-equal between the full
    launch and its clipped twins on the rows and columns (ln_part: the 128-column slabs) both hold."""
    a, w, bias, x0, mean_prev, (ref, bound) = producer_operands(K, dtype)
    runs = {}
    for M, Nn in GROUPS[K]:
        for half_m in (-1, 1):
            out, h16, part = run_producer(a[:M].contiguous(), w[:Nn].contiguous(), bias[:Nn].contiguous(), x0[:M, :Nn].contiguous(),
                                          mean_prev[:M], half_m)
            f_out = frac((out.double() - ref[:M, :Nn]).abs(), bound[:M, :Nn])
            _, h_ref, p_ref, p_bound = R.producer_side(out, mean_prev[:M], dtype)
            err = (part.double() - p_ref).abs()
            f_s1 = frac(err[..., 0], p_bound[..., 0].clamp_min(1e-30))
            f_s2 = frac(err[..., 1], p_bound[..., 1].clamp_min(1e-30))
            print(f"\nproducer ({M},{Nn},{K}) half_m={half_m} {dtype}: out {f_out:.3f}, S1 {f_s1:.3f}, S2 {f_s2:.3f} of the bound")
            assert f_out <= 1.0 and bool((err <= p_bound).all()), (M, Nn, half_m, f_out, f_s1, f_s2)
            assert same_bits(h16, h_ref)
            runs[(M, Nn, half_m)] = (out, h16, part)
        for x, y in zip(runs[(M, Nn, -1)], runs[(M, Nn, 1)]):
            assert same_bits(x, y), f"({M},{Nn}): the two tile heights differ"
    M0, N0 = GROUPS[K][0]
    for M, Nn in GROUPS[K][1:]:
        m, n = min(M, M0), min(Nn, N0)
        for half_m in (-1, 1):
            o0, h0, p0 = runs[(M0, N0, half_m)]
            o1, h1, p1 = runs[(M, Nn, half_m)]
            assert same_bits(o1[:m, :n], o0[:m, :n]) and same_bits(h1[:m, :n], h0[:m, :n]), f"full and clipped ({M},{Nn}) differ"
            assert same_bits(p1[:m, : n // 128], p0[:m, : n // 128]), f"ln_part of full and clipped ({M},{Nn}) differ"


# ---- two tiles per workgroup --------------------------------------------------------------------------------------------------
M2, N2 = 4352, 4096  # 17 x 16 = 272 full tiles on 256 workgroups


def gpu_randn(*shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with2", [False, True], ids=["bias", "bias+bias2"])
@pytest.mark.parametrize("half_m", [1, -1])
@pytest.mark.parametrize("K", [64, 192])
def test_consumer_two_tiles_per_workgroup(K, half_m, with2, dtype):
    a = gpu_randn(M2, K, seed=K).to(dtype)
    w = (gpu_randn(N2, K, seed=K + 1) / math.sqrt(K)).to(dtype)
    bias = gpu_randn(N2, seed=K + 2)
    bias2 = gpu_randn(N2, seed=K + 3) if with2 else None
    rstd = 0.05 * (300 / 0.05) ** torch.rand(M2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K + 4))
    whole = run_consumer(a, w, bias, bias2, rstd, half_m)
    for s in range(0, M2, 256):
        alone = run_consumer(a[s:s + 256].contiguous(), w, bias, bias2, rstd[s:s + 256], half_m)
        assert same_bits(whole[s:s + 256], alone), f"rows {s} .. {s + 255} differ from the slice launched alone"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("half_m", [1, -1])
@pytest.mark.parametrize("K", [64, 192])
def test_producer_two_tiles_per_workgroup(K, half_m, dtype):
    a = gpu_randn(M2, K, seed=K + 10).to(dtype)
    w = (gpu_randn(N2, K, seed=K + 11) / math.sqrt(K)).to(dtype)
    bias = gpu_randn(N2, seed=K + 12)
    x0 = 3 * gpu_randn(M2, N2, seed=K + 13) + 0.7
    mean = 0.7 + 0.1 * gpu_randn(M2, seed=K + 14)
    out, h16, part = run_producer(a, w, bias, x0, mean, half_m)
    for s in range(0, M2, 256):
        o1, h1, p1 = run_producer(a[s:s + 256].contiguous(), w, bias, x0[s:s + 256].contiguous(), mean[s:s + 256], half_m)
        assert same_bits(out[s:s + 256], o1) and same_bits(h16[s:s + 256], h1) and same_bits(part[s:s + 256], p1), \
            f"rows {s} .. {s + 255} differ from the slice launched alone"
