"""tests/_dense_gemm_ref.py pinned without a GPU: the reference must be able to fail.

A correct kernel is emulated on the CPU: the fp32 torch matmul of the same operands, the epilogue in fp32, rounded to the
output dtype.  It stays within expected()'s bound at every shape with M <= 300, every epilogue, both dtypes, with and
without a bias; on the exact case it equals the fp64 result bit for bit.  Then the emulation is broken in the ways a
tiled kernel breaks, and each fault must pass the bound in at least one element of the region it touches (and, for (a) -
(d) and (f), break the exact case's torch.equal):
    (a) k_chunk   the last 32-column K chunk left out for the rows of the clipped last 128-row wave block
    (b) rows      rows m and m + 16 exchanged inside the last row block that holds more than 16 rows (M > 16)
    (c) bias      no bias on the N-tail columns (the last, partly filled 128-column wave block)
    (d) resid     EPI_RESID_F32: the residual dropped, or added twice, in the last row
    (e) trunc     EPI_STORE_T: the store truncates toward zero instead of rounding to nearest
    (f) columns   columns n and n + 128 exchanged (N > 128)

(e) in figures.  G.store allows UNIT |y|, between half an ulp and a whole one across a binade, so a truncation error t
(uniform over [0, 1) ulp) passes the bound where t > |y| / 2^(e+1) + accumulation bound: a quarter to a third of the
elements (the mean of 1 - f over a binade) while the accumulation bound is small against the ulp, fewer as it grows.  The
accumulation bound over UNIT |y| is about 2 (K + 1) 2^-24 0.64 sqrt(K) / (UNIT |y|): 0.01 / |y| for bf16 and 0.08 / |y|
for fp16 at K = 64, 0.11 / |y| and 0.9 / |y| at K = 320 — with |y| of order 1 not "far below" the fp16 ulp at the longer
K, so fewer fp16 elements fail there.  The test requires a tenth of all elements in bf16 and in fp16 at K <= 128, and a
fiftieth in fp16 at the longer K; it prints the count.  MEASURED, share of all elements fp16 / bf16: (1, 8, 64) 2 of 8 /
2 of 8; (255, 136, 128) 0.121 / 0.232; (130, 200, 96) 0.151 / 0.246; (128, 264, 192) 0.074 / 0.215 (2516 / 7265 elements);
(300, 384, 256) 0.044 / 0.191 (5038 / 21994); (77, 33, 320) 0.027 / 0.181 (69 / 461 of 2541)."""
import pytest
import torch

import _dense_gemm_ref as D

DTYPES = list(D.DTYPES)
IDS = ["fp16", "bf16"]
CPU_SHAPES = [s for s in D.EDGE_SHAPES + D.GENERIC_SHAPES if s[0] <= 300]
GENERIC = set(D.GENERIC_SHAPES)
BOUND_MUTATIONS = ["k_chunk", "rows", "bias", "resid_dropped", "resid_twice", "columns"]


def truncate(v, dtype):
    """fp32 -> dtype toward zero (round to nearest, then step back where that went away from zero)"""
    r = v.to(dtype)
    away = r.float().abs() > v.abs()
    zero = torch.zeros((), dtype=dtype)
    return torch.where(away, torch.nextafter(r, zero), r)


def swap_rows(t, lo, hi):
    """rows m and m + 16 exchanged for every m of [lo, hi) with m % 32 < 16 and m + 16 < hi"""
    t = t.clone()
    m = torch.arange(lo, hi)
    m = m[((m - lo) % 32 < 16) & (m + 16 < hi)]
    t[m], t[m + 16] = t[m + 16].clone(), t[m].clone()
    return t, torch.cat([m, m + 16])


def swap_columns(t):
    t = t.clone()
    n = torch.arange(t.shape[1])
    n = n[(n % 256 < 128) & (n + 128 < t.shape[1])]
    t[:, n], t[:, n + 128] = t[:, n + 128].clone(), t[:, n].clone()
    return t, torch.cat([n, n + 128])


def emulate(epi, a, w, bias, resid, mut=None):
    """(what a correct fp32-accumulating kernel stores, or the fault `mut` of it; mask [M,N] of the region touched)"""
    M, K = a.shape
    Nn = w.shape[0]
    dtype = a.dtype
    region = torch.zeros(M, Nn, dtype=torch.bool)
    acc = a.float() @ w.float().T
    if mut == "k_chunk":
        r0 = D.last_row_block(M)
        acc[r0:] = a[r0:, :K - 32].float() @ w[:, :K - 32].float().T
        region[r0:] = True
    if bias is not None:
        b = bias.clone()
        if mut == "bias":
            b[D.n_tail_start(Nn):] = 0
            region[:, D.n_tail_start(Nn):] = True
        acc = acc + b
    if epi in (D.EPI_GELU_T, D.EPI_GELU_F32):
        acc = torch.nn.functional.gelu(acc)
    if epi == D.EPI_RESID_F32:
        r = resid.clone()
        if mut == "resid_dropped":
            r[M - 1] = 0
        if mut == "resid_twice":
            r[M - 1] *= 2
        if mut in ("resid_dropped", "resid_twice"):
            region[M - 1] = True
        acc = r + acc
    if mut == "rows":
        r0 = D.last_row_block(M)
        if M - r0 <= 16:
            r0 -= 128
        acc, rows = swap_rows(acc, r0, min(r0 + 128, M))
        region[rows] = True
    if mut == "columns":
        acc, cols = swap_columns(acc)
        region[:, cols] = True
    odt = D.out_dtype(epi, dtype)
    out = truncate(acc, odt) if mut == "trunc" else acc.to(odt)
    if mut == "trunc":
        region[:] = True
    return out, region


def applies(mut, epi, M, Nn, with_bias):
    if mut == "rows":
        return M > 16
    if mut == "columns":
        return Nn > 128
    if mut == "bias":
        return with_bias
    if mut in ("resid_dropped", "resid_twice"):
        return epi == D.EPI_RESID_F32
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,Nn,K", CPU_SHAPES)
def test_fp32_emulation_is_within_the_bound_and_every_fault_passes_it(M, Nn, K, dtype):
    a, w, bias, resid = D.case(M, Nn, K, dtype, seed=M + Nn + K)
    generic = (M, Nn, K) in GENERIC
    worst = 0.0
    for with_bias in (True, False):
        bs = bias if with_bias else None
        for epi in D.EPILOGUES:
            val, bound = D.expected(epi, a, w, bs, resid, generic=generic)
            got, _ = emulate(epi, a, w, bs, resid)
            frac = ((got.double() - val).abs() / bound).max().item()
            worst = max(worst, frac)
            assert frac <= 1.0, (D.EPI_NAMES[epi], with_bias, frac)
            for mut in BOUND_MUTATIONS:
                if not applies(mut, epi, M, Nn, with_bias):
                    continue
                bad, region = emulate(epi, a, w, bs, resid, mut)
                assert region.any(), mut
                fails = ((bad.double() - val).abs() > bound) & region
                assert fails.any(), (mut, D.EPI_NAMES[epi], with_bias)
    print(f"\n{M} x {Nn} x {K} {dtype}: the emulation reaches {worst:.3f} of its bound")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,Nn,K", [s for s in CPU_SHAPES if s[2] <= 320])
def test_a_truncating_store_fails_a_sizeable_share(M, Nn, K, dtype):
    a, w, bias, resid = D.case(M, Nn, K, dtype, seed=M + Nn + K)
    val, bound = D.expected(D.EPI_STORE_T, a, w, bias, resid)
    bad, _ = emulate(D.EPI_STORE_T, a, w, bias, resid, "trunc")
    fails = (bad.double() - val).abs() > bound
    share = fails.double().mean().item()
    print(f"\ntruncating store {M} x {Nn} x {K} {dtype}: {int(fails.sum())} of {fails.numel()} elements fail ({share:.3f})")
    need = 0.1 if dtype == torch.bfloat16 or K <= 128 else 0.02
    assert share >= need and fails.sum().item() >= 2, share


def test_truncate_is_toward_zero():
    v = torch.tensor([1.0009765625, -1.0009765625, 1.0, -3.0, 65504.0, 1e-9, -1e-9, 0.0], dtype=torch.float32) * 1.0001
    for dtype in DTYPES:
        t = truncate(v, dtype).float()
        assert (t.abs() <= v.abs()).all() and (t.sign() * v.sign() >= 0).all()
        up = torch.nextafter(t.to(dtype), (v.sign() * float("inf")).to(dtype)).float()
        assert (up.abs() > v.abs())[v != 0].all()  # the next value away from zero is past v: t is the nearest below


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,Nn,K", CPU_SHAPES)
def test_exact_case_is_bit_equal_and_catches_every_fault(M, Nn, K, dtype):
    K = D.exact_k(K, dtype)
    a, w, bias, resid = D.exact_case(M, Nn, K, dtype)
    for with_bias in (True, False):
        bs = bias if with_bias else None
        for epi in D.EXACT_EPILOGUES:
            want = D.exact_expected(epi, a, w, bs, resid)
            got, _ = emulate(epi, a, w, bs, resid)
            assert got.dtype == want.dtype and torch.equal(got, want), (D.EPI_NAMES[epi], with_bias)
            for mut in BOUND_MUTATIONS:
                if not applies(mut, epi, M, Nn, with_bias):
                    continue
                bad, region = emulate(epi, a, w, bs, resid, mut)
                assert not torch.equal(bad, want), (mut, D.EPI_NAMES[epi], with_bias)
                assert torch.equal(bad[~region], want[~region])  # and nothing outside the region moved
        for epi in (D.EPI_GELU_T, D.EPI_GELU_F32):  # the GELU epilogues: the bound, on exactly known pre-activations
            val, bound = D.expected(epi, a, w, bs, resid)
            got, _ = emulate(epi, a, w, bs, resid)
            assert ((got.double() - val).abs() <= bound).all()


def test_exact_case_refuses_a_k_the_dtype_cannot_hold():
    with pytest.raises(AssertionError):
        D.exact_case(4, 8, 128, torch.bfloat16)
    with pytest.raises(AssertionError):
        D.exact_case(4, 8, 1024, torch.float16)
    D.exact_case(4, 8, 960, torch.float16)


def test_shape_tables_meet_their_conditions():
    for M, Nn, K, tile_m in D.SEAM_SHAPES:
        assert D.is_seam(M, Nn, K, tile_m) and K % 64 == 0, (M, Nn, K)
    assert {s[2] // 64 for s in D.SEAM_SHAPES} == {1, 5}
    for M, Nn, K in D.EDGE_SHAPES:
        assert K % 64 == 0 and Nn % 8 == 0  # every tiled kernel takes them
    (_, n1, k1), (_, n2, k2) = D.GENERIC_SHAPES
    assert n1 % 4 != 0 and k2 % 64 != 0 and k1 % 32 == 0 and k2 % 32 == 0
    assert D.n_tail_start(8) == 0 and D.n_tail_start(264) == 256 and D.n_tail_start(136) == 128 and D.n_tail_start(384) == 256
    assert D.last_row_block(129) == 128 and D.last_row_block(128) == 0 and D.last_row_block(1) == 0
