"""The GELU of every GEMM launcher that has one (reference esm/modules.py:17-24), swept on the device over pre-activations
that are known EXACTLY: signed zeros, fp32 denormals, +-1e-8, +-1e-3, a linspace over [-12, 12], the two fp32 neighbours
on either side of +-4 and +-4.75 (the clamps of the two coefficient sets of esm_amd/csrc/common.h gelu_fast), +-100, +-1e4
and, for bf16 / fp32 outputs, +6e4.  The other GPU tests feed random pre-activations that rarely pass |x| = 4 and compare
against a tolerance relative to max |ref|: a wrong clamp constant, the other coefficient set in one instantiation or a
broken negative tail pass them.

Two feeds, M = 130 rows (a clipped second wave block), N = the 2048 grid points:
  * bias: a = 0 and the grid in the bias — the pre-activation is the bias itself, and every row must be bit-identical to row 0;
  * product: no bias, K = 64, a[m, 0] = 2^(m % 3 - 1), w[n, 0] = the grid rounded to the operand dtype: the products are exact.
Bounds against gelu64 of the exact pre-activation (tests/_ln_fold_ref.py: the figures tests/test_host_cpu.py asserts for
the coefficient sets) plus half an ulp of the output dtype:
  * fp32 set (degree 11, clamp 4.75): 2e-6 inside the clamp, 2e-6 |x| beyond;
  * operand-dtype set (degree 8, clamp 4): 8e-6 inside, 3.2e-5 |x| beyond, never positive left of the clamp — and at
    x <= -100 the residue is at least 2.8e-5 |x| (1 - Phi(4) = 3.17e-5 less the 2e-6 the fit may be off at the clamp, less
    a bf16 rounding), which the fp32 set (<= 2e-6 |x|) cannot produce: each set is told from the other in both directions;
  * erff: the allowance of tests/test_precision_ops_gpu.py::test_linear_f32 — 4 x the error of torch's fp32 gelu against
    gelu64 on the same points, in units of 2^-24 max(1, |x|).

Which set each launcher was FOUND to use (by the code, confirmed by the bounds on an MI355X):
    ops.linear EPI_GELU_T:   gemm9 full / half height, gemm8, force_old (gemm256)   operand-dtype set;  force_generic: erff
    ops.linear EPI_GELU_F32: gemm9 full / half height, gemm8, force_old             fp32 set;           force_generic: erff
    ops.linear_gelu_x3 (hi | hi | lo rows, hi + lo checked): fp32 set;   ops.linear_f32(gelu=True): erff
    the LayerNorm-fold consumer (esmk_op_linear_ln, epilogue 2; rstd a power of two): operand-dtype set

MEASURED on an MI355X, largest error as a fraction of the bound (bias / product feed), printed by every case (`pytest -s`):
    EPI_GELU_T, operand-dtype set: gemm9 full / half, gemm8, force_old, fold consumer   0.998 / 0.995 fp16, 0.997 / 0.993 bf16
                                   (the half ulp of the store; 0.934 of the bound where the store is below a tenth of it:
                                   the function alone, 7.5e-6 of the 8e-6)
    EPI_GELU_F32, fp32 set:        gemm9 full / half, gemm8, force_old                   0.607 / 0.607
    linear_gelu_x3, fp32 set:      0.594 / 0.583
    erff:                          force_generic fp32 out 0.220 / 0.224, 16-bit out 0.998 / 0.997; linear_f32 0.220 / 0.226
"""
import ctypes

import pytest
import torch

import _ln_fold_ref as R
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu

M, K, NGRID = 130, 64, 2048
G = 2
SENT = 7.0
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def grid(big):
    """fp32 [2048] on the GPU: the special points and a linspace over [-12, 12]; big: with +6e4"""
    sp = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e-8, -1e-8, 1e-3, -1e-3, 100.0, -100.0, 1e4, -1e4]
    for c in (4.0, 4.75):
        for s in (1.0, -1.0):
            v = torch.tensor(s * c, dtype=torch.float32)
            up, dn = v.clone(), v.clone()
            sp.append(v.item())
            for _ in range(2):
                up = torch.nextafter(up, torch.tensor(float("inf")))
                dn = torch.nextafter(dn, torch.tensor(float("-inf")))
                sp += [up.item(), dn.item()]
    if big:
        sp.append(6e4)
    t = torch.cat([torch.tensor(sp, dtype=torch.float32), torch.linspace(-12, 12, NGRID - len(sp), dtype=torch.float32)])
    assert t.numel() == NGRID and torch.isfinite(t).all()
    return t.cuda()


# name -> (keywords of ops.linear, flags of esmk_debug_gemm_plan, planned kernel, polynomial or erff)
LAUNCHERS = {
    "gemm9_full": ({"half_m": -1}, 0, 9, "poly"),
    "gemm9_half": ({"half_m": 1}, 0, 9, "poly"),
    "gemm8": ({}, 0, 8, "poly"),
    "force_old": ({"force_old": True}, 2, 256, "poly"),
    "force_generic": ({"force_generic": True}, 1, 64, "erff"),
}


@pytest.fixture
def gemm8_impl():
    N.check(N.lib.esmk_debug_gemm_impl(8, 0))
    yield
    N.check(N.lib.esmk_debug_gemm_impl(0, 0))


def plan(epi, flags):
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, NGRID, K, epi, flags, out))
    return out[0]


def feeds(op_dtype, big, need_bias=False):
    """(name, a [M,K], w [N,K], bias or None, exact fp64 pre-activation [M,N]) of the two feeds"""
    gr = grid(big)
    a0 = torch.zeros(M, K, dtype=op_dtype, device="cuda")
    w0 = torch.zeros(NGRID, K, dtype=op_dtype, device="cuda")
    w0[:, 1] = 1  # a finite weight that the zero activations must silence
    yield "bias", a0, w0, gr, gr.double()[None, :].expand(M, NGRID)
    a = torch.zeros(M, K, dtype=op_dtype, device="cuda")
    a[:, 0] = 2.0 ** (torch.arange(M, device="cuda") % 3 - 1)
    w = torch.zeros(NGRID, K, dtype=op_dtype, device="cuda")
    w[:, 0] = gr.to(op_dtype)
    zero = torch.zeros(NGRID, device="cuda") if need_bias else None
    yield "product", a, w, zero, a[:, :1].double() * w[:, 0].double()[None, :]


def check(name, feed, got, pre, out_dtype, cset, half=None):
    """got fp64 [M,N] against gelu64(pre) within the bound of the coefficient set + half an ulp (`half`: its own rule)"""
    assert torch.isfinite(got).all()
    val = R.gelu64(pre)
    if cset == "erff":
        unit = R.U * pre.abs().clamp(min=1.0)
        erf_meas = ((torch.nn.functional.gelu(pre.float()).double() - val).abs() / unit).max().item()
        assert erf_meas > 0
        b = 4 * erf_meas * unit
    else:
        b = R.gelu_poly_bound(pre, cset == "t16")
    store = R.half_ulp(val.abs() + b, out_dtype) if half is None else half(val, b)
    allow = b + store
    err = (got - val).abs()
    f = (err / allow).max().item()
    fine = store < 0.1 * b  # where the store is fine against the function's own bound, the figure is the function's
    f_fn = (err / allow)[fine].max().item() if fine.any() else float("nan")
    print(f"\ngelu {name} [{feed}] -> {out_dtype}, {cset}: {f:.3f} of the bound ({f_fn:.3f} where the store is < 0.1 of it)")
    assert f <= 1.0, (name, feed, f)
    if cset == "t16":
        clamp = R.GELU_SETS[True][0]
        assert (got[pre < -clamp] <= 0).all(), "positive value on the left tail"
        far = pre <= -100
        assert far.any() and (-got[far] >= 2.8e-5 * pre[far].abs()).all(), "not the operand-dtype set's tail"
    if feed == "bias":
        assert bool((got == got[:1]).all()), "rows differ on the same pre-activation"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("epi", [N.EPI_GELU_T, N.EPI_GELU_F32], ids=["gelu_t", "gelu_f32"])
@pytest.mark.parametrize("name", ["gemm9_full", "gemm9_half", "force_old", "force_generic"])
def test_linear_gelu(name, epi, dtype):
    run_linear(name, epi, dtype)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("epi", [N.EPI_GELU_T, N.EPI_GELU_F32], ids=["gelu_t", "gelu_f32"])
def test_linear_gelu_gemm8(epi, dtype, gemm8_impl):
    run_linear("gemm8", epi, dtype)


def run_linear(name, epi, dtype):
    kw, flags, kernel, cset = LAUNCHERS[name]
    assert plan(epi, flags) == kernel
    out_dtype = dtype if epi == N.EPI_GELU_T else F32
    if cset == "poly":
        cset = "t16" if epi == N.EPI_GELU_T else "f32"
    for feed, a, w, bias, pre in feeds(dtype, big=out_dtype != F16):
        out = ops.linear(a, w, bias, epi, out=torch.full((M + G, NGRID), SENT, dtype=out_dtype, device="cuda"), **kw)
        assert bool((out[M:] == SENT).all()), "stray store"
        check(name, feed, out[:M].double(), pre, out_dtype, cset)


def test_linear_gelu_x3():
    """fc1 + GELU of the f16x3 mode: rows hi | hi | lo per 64 columns; hi + lo carries the value to 2^-22 |v| (lo = fp16(v -
    hi) is rounded to 11 bits of a value below 2^-11 |v|) or to half the subnormal spacing 2^-25"""
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, NGRID, K, N.EPI_GELU_T, 32, out))
    assert out[0] == 9
    for feed, a, w, bias, pre in feeds(F16, big=False, need_bias=True):
        a3 = torch.cat([a, a, torch.zeros_like(a)], 1)  # hi | hi | lo of the one 64-column K tile
        w3 = torch.cat([w, torch.zeros_like(w), w], 1)  # hi | lo | hi
        out3 = torch.full((M + G, 3 * NGRID), SENT, dtype=F16, device="cuda")
        ops.linear_gelu_x3(a3, w3, bias, out3=out3, M=M)
        assert bool((out3[M:] == SENT).all()), "stray store"
        blocks = out3[:M].view(M, NGRID // 64, 3, 64)
        assert torch.equal(blocks[:, :, 0], blocks[:, :, 1])
        got = (blocks[:, :, 0].double() + blocks[:, :, 2].double()).reshape(M, NGRID)
        check("linear_gelu_x3", feed, got, pre, F16, "f32", half=lambda val, b: 2.0 ** -22 * (val.abs() + b) + 2.0 ** -25)


def test_linear_f32_gelu():
    for feed, a, w, bias, pre in feeds(F32, big=True):
        out = torch.full((M + G, NGRID), SENT, device="cuda")
        ops.linear_f32(a, w, bias, gelu=True, out=out, M=M)
        assert bool((out[M:] == SENT).all()), "stray store"
        check("linear_f32", feed, out[:M].double(), pre, F32, "erff")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("half_m", [1, -1])
def test_fold_consumer_gelu(half_m, dtype):
    """esmk_op_linear_ln, epilogue 2: value = fma(acc, rstd, bias + bias2) with rstd = 2 / 0.5 by row — still exact"""
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, NGRID, K, N.EPI_GELU_T, 4, out))
    assert out[0] == 9
    rstd = torch.full((256,), float("nan"), device="cuda")
    rstd[:M] = 2.0 ** (1 - 2 * (torch.arange(M, device="cuda") % 2))
    for feed, a, w, bias, pre in feeds(dtype, big=dtype != F16, need_bias=True):
        if feed == "product":
            a[:, 0] = 1  # rstd * w <= 2e4 in fp16
            pre = rstd[:M, None].double() * w[:, 0].double()[None, :]
        got = torch.full((M + G, NGRID), SENT, dtype=dtype, device="cuda")
        N.check(N.lib.esmk_op_linear_ln(N.ptr(a), N.ptr(w), N.ptr(bias), None, N.ptr(got), M, NGRID, K, N.EPI_GELU_T,
                                        R.DT_CODE[dtype], N.ptr(rstd), None, 0, None, 0, None, half_m, N.cur_stream()))
        assert bool((got[M:] == SENT).all()), "stray store"
        check(f"fold consumer half_m={half_m}", feed, got[:M].double(), pre, dtype, "t16")
