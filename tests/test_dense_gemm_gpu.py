"""The dense GEMM kernels behind ops.linear, one launch at a time against fp64 (tests/_dense_gemm_ref.py): gemm9 with
full-height and half-height tiles, gemm8 with both (what ESMK_GEMM_IMPL=8 ships), the 256 x 256 tile kernel and the
generic 64 x 64 kernel, with the five plain epilogues, with and without a bias, fp16 and bf16.  The other dense tests
(tests/test_kernels_gpu.py) compare with an fp32 matmul under one global tolerance, or the kernels with each other — which
share gemm_epi.h, the bias-as-C-operand convention and the store helpers.

Every case
  * asserts the planned kernel (esmk_debug_gemm_plan with the case's flags and impl setting) before it launches;
  * writes through out = rows [G, G + M) of a buffer of M + 2 G rows filled with a NaN bit pattern (for EPI_RESID_F32 the
    view holds the residual): the guard rows must keep that pattern bit for bit, and after a store epilogue no element
    of the view may still hold it.  G = 256: every row a clipped tile could reach;
  * holds every element to |got - value| <= bound of the fp64 reference computed on the device from the same tensors,
    and reports the worst element with the tile and wave block it lies in;
  * runs the exact case (small-integer operands, K cut to what the dtype holds) at the non-seam shapes: the three
    epilogues without a GELU must equal the fp64 result BIT FOR BIT, the two with one stay within their bound.
Shapes: tests/_dense_gemm_ref.py EDGE_SHAPES, SEAM_SHAPES (306 tiles on 256 workgroups: the K-tile stream crosses a tile
seam with 1 and 5 K tiles; not for the generic kernel, which has no persistence) and GENERIC_SHAPES.

MEASURED on an MI355X, the largest error as a fraction of its bound over all shapes (`pytest -s` prints it per case):
                                           store_t   store_f32   gelu_t   gelu_f32   resid_f32
    gemm9 full / half, gemm8 full / half,
    gemm256 (the same bits)         fp16    0.976      0.022     0.966     0.103      0.025
                                    bf16    0.993      0.022     0.995     0.106      0.025
    gemm64                          fp16    0.923      0.008     0.925     0.006      0.008
                                    bf16    0.980      0.006     0.988     0.006      0.008
The operand-dtype epilogues sit near 1 because their bound is the rounding of the store itself (a truncating store passes
it in 3 - 25 % of the elements, tests/test_dense_gemm_reference_cpu.py); the fp32 epilogues use a few hundredths of a
worst-case accumulation bound (at K = 5120 below 0.001 of it), so there the exact case is the sharper check: every
kernel, epilogue and shape was bit-equal.  No stray store and no missing store in any case.
"""
import ctypes

import pytest
import torch

import _dense_gemm_ref as D
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu

G_ROWS = 256
SENTINEL = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float16: (torch.int16, 0x7E5A), torch.bfloat16: (torch.int16, 0x7FDA)}

# name -> (keywords of ops.linear, impl of esmk_debug_gemm_impl, flags of esmk_debug_gemm_plan, planned kernel, tile rows, tile columns)
KERNELS = {
    "gemm9_full": ({"half_m": -1}, 0, 0, 9, 256, 256),
    "gemm9_half": ({"half_m": 1}, 0, 0, 9, 128, 256),
    "gemm8_full": ({"half_m": -1}, 8, 0, 8, 256, 256),
    "gemm8_half": ({"half_m": 1}, 8, 0, 8, 128, 256),
    "gemm256": ({"force_old": True}, 0, 2, 256, 256, 256),
    "gemm64": ({"force_generic": True}, 0, 1, 64, 64, 64),
}


SEAM = {s[:3] for s in D.SEAM_SHAPES}


def cases():
    out = []
    for dtype, dname in zip(D.DTYPES, ("fp16", "bf16")):
        for shape in D.EDGE_SHAPES + tuple(s[:3] for s in D.SEAM_SHAPES) + D.GENERIC_SHAPES:
            for kernel in KERNELS:
                if shape in D.GENERIC_SHAPES and kernel != "gemm64":
                    continue
                if kernel == "gemm64" and shape in SEAM:  # the seam shapes test persistence: the generic kernel has none
                    continue
                out.append(pytest.param(dtype, shape, kernel, id=f"{dname}-{shape[0]}x{shape[1]}x{shape[2]}-{kernel}"))
    return out


@pytest.fixture(autouse=True)
def _restore_impl():
    yield
    N.check(N.lib.esmk_debug_gemm_impl(0, 0))


def test_epilogue_codes_are_the_library_s():
    assert (N.EPI_STORE_T, N.EPI_STORE_F32, N.EPI_GELU_T, N.EPI_GELU_F32, N.EPI_RESID_F32) == D.EPILOGUES


def planned(M, Nn, K, epi, flags):
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, Nn, K, epi, flags, out))
    return out[0]


def guarded(M, Nn, dtype, resid=None):
    """(buffer [M + 2 G, N] of the sentinel pattern, its rows [G, G + M), the sentinel as the integer view holds it)"""
    it, pattern = SENTINEL[dtype]
    buf = torch.full((M + 2 * G_ROWS, Nn), pattern, dtype=it, device="cuda").view(dtype)
    view = buf[G_ROWS:G_ROWS + M]
    if resid is not None:
        view.copy_(resid)
    return buf, view, it, pattern


def launch(kernel, epi, a, w, bias, resid):
    """ops.linear into a guarded view; the guards checked, the view returned"""
    kw = KERNELS[kernel][0]
    M, Nn = a.shape[0], w.shape[0]
    odt = D.out_dtype(epi, a.dtype)
    buf, view, it, pattern = guarded(M, Nn, odt, resid if epi == D.EPI_RESID_F32 else None)
    ops.linear(a, w, bias, epi, out=view, **kw)
    bits = buf.view(it)
    for name, rows in (("before", bits[:G_ROWS]), ("after", bits[G_ROWS + M:])):
        stray = (rows != pattern).nonzero()
        assert stray.numel() == 0, (f"{kernel} {D.EPI_NAMES[epi]}: {stray.shape[0]} stray stores in the guard rows {name} the "
                                    f"output, the first at guard row {stray[0, 0].item()}, column {stray[0, 1].item()}")
    if epi != D.EPI_RESID_F32:
        left = (bits[G_ROWS:G_ROWS + M] == pattern).nonzero()
        assert left.numel() == 0, (f"{kernel} {D.EPI_NAMES[epi]}: {left.shape[0]} elements never stored, the first at "
                                   f"({left[0, 0].item()}, {left[0, 1].item()})")
    return view


def check_bound(kernel, epi, with_bias, got, val, bound):
    tile_m, tile_n = KERNELS[kernel][4:]
    got = got.double()
    assert torch.isfinite(got).all(), f"{kernel} {D.EPI_NAMES[epi]}: non-finite output"
    frac = (got - val).abs() / bound
    worst = frac.argmax().item()
    m, n = divmod(worst, got.shape[1])
    f = frac[m, n].item()
    assert f <= 1.0, (f"{kernel} {D.EPI_NAMES[epi]} bias={with_bias}: element ({m}, {n}) is {got[m, n].item():.9g}, fp64 "
                      f"{val[m, n].item():.9g}: error {abs(got[m, n].item() - val[m, n].item()):.3e} against the bound "
                      f"{bound[m, n].item():.3e} ({f:.2f} of it); {int((frac > 1).sum())} elements fail; {D.where(m, n, tile_m, tile_n)}")
    return f


def check_equal(kernel, epi, with_bias, got, want):
    tile_m, tile_n = KERNELS[kernel][4:]
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    m, n = bad[0].tolist()
    raise AssertionError(f"{kernel} {D.EPI_NAMES[epi]} bias={with_bias}, exact case: {bad.shape[0]} elements differ, the first "
                         f"({m}, {n}): {got[m, n].item()} for {want[m, n].item()}; rows {bad[:, 0].min().item()}..{bad[:, 0].max().item()}, "
                         f"columns {bad[:, 1].min().item()}..{bad[:, 1].max().item()}; {D.where(m, n, tile_m, tile_n)}")


@pytest.mark.parametrize("dtype,shape,kernel", cases())
def test_dense_gemm_against_fp64(dtype, shape, kernel):
    M, Nn, K = shape
    _, impl, flags, want_kernel, _, _ = KERNELS[kernel]
    generic = kernel == "gemm64"
    N.check(N.lib.esmk_debug_gemm_impl(impl, 0))
    for epi in D.EPILOGUES:
        assert planned(M, Nn, K, epi, flags) == want_kernel, (kernel, D.EPI_NAMES[epi])
    a, w, bias, resid = D.case(M, Nn, K, dtype, seed=M + Nn + K, device="cuda")
    worst = {}
    for with_bias in (True, False):
        bs = bias if with_bias else None
        for epi in D.EPILOGUES:
            got = launch(kernel, epi, a, w, bs, resid)
            val, bound = D.expected(epi, a, w, bs, resid, generic=generic)
            f = check_bound(kernel, epi, with_bias, got, val, bound)
            worst[epi] = max(worst.get(epi, 0.0), f)
            del val, bound, got
    print(f"\ndense {kernel} {M} x {Nn} x {K} {dtype}: " + ", ".join(f"{D.EPI_NAMES[e]} {worst[e]:.3f}" for e in D.EPILOGUES)
          + " of the bound")
    if shape in SEAM:
        return
    Ke = D.exact_k(K, dtype)
    for epi in D.EPILOGUES:
        assert planned(M, Nn, Ke, epi, flags) == want_kernel, (kernel, D.EPI_NAMES[epi], "exact case")
    a, w, bias, resid = D.exact_case(M, Nn, Ke, dtype, device="cuda")
    for with_bias in (True, False):
        bs = bias if with_bias else None
        for epi in D.EPILOGUES:
            got = launch(kernel, epi, a, w, bs, resid)
            if epi in D.EXACT_EPILOGUES:
                check_equal(kernel, epi, with_bias, got, D.exact_expected(epi, a, w, bs, resid))
            else:
                val, bound = D.expected(epi, a, w, bs, resid, generic=generic)
                check_bound(kernel, epi, with_bias, got, val, bound)
