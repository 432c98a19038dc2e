"""One launch of each kernel family at the smallest shape whose addresses pass 2^31 and 2^32 bytes (and 2^31 elements),
every output element checked (tests/_index_width.py: chunk equality over all rows, the op's fp64 reference on the rows
around each boundary, sentinel and guard rows).  The arithmetic is not under test: K = 64 (or the smallest the entry
takes), T = 64.

Families here: the dense GEMM kernels behind ops.linear (gemm9, gemm8, the 256 x 256 and the 64 x 64 kernel; the five
plain epilogues; the A operand), f16x2 (ops.linear_split) and f16x3 (ops.linear_gelu_x3), the attention core for
head_dim 64 and 128 (plain, and the padded form with seq_info on a chunk-sized subset), token-packed attention, the
padded attention maps (head_dim 64 and 128), the MSA column maps, the unfused and the fused contact head, the pair head,
gemm9's q / k (RoPE) and V^T epilogues in one and two launches, plain and with the LayerNorm fold, the fold's producer
and consumer epilogues (esmk_op_linear_ln), the LayerNorm launches of the layer loop (engine form and variant 0, ldy = E
and ldy > E) and its other row kernels: embed, add_positions, scale_rows, zero_gap_rows, rowstats, gather_rows,
blend_rows, pool_rows, sae_rows, align_rows, masked_row_mean, stream_edit.
Attention, LayerNorm and the unfused contact head go through the C entries that the ops wrappers call, because those
wrappers allocate their outputs themselves and a sentinel needs the caller's buffer.

NOT COVERED, here or in tests/test_index_width_engine_gpu.py:
    head_dim-128 q / k / v epilogues   the single-op entries refuse head_dim != 64, and at 15B dims with B 104 q, k and V^T
                                       are 1.09 GB each: they cross in no test
    token-packed maps and contacts     ops.attention_probs_packed (tests/test_varlen_maps_gpu.py takes its map offsets
                                       past 2^31 elements) and the packed form of ops.contacts_fused
    ops.attention_biaskv, the f16x3 context layout of ops.attention, the MSA row-attention forms of ops.gemm_ex and
    ops.msa_row_softmax, the reduced-precision (operand dtype) map outputs
Out of scope, because they stay small at every shape the entries accept:
    weights and their images   N, K <= 20480: 20480 * 20480 * 2 * 3 bytes = 2.3 GiB is the f16x3 fc image only; every
                               other weight is below 2^31 bytes, and none is indexed by a row count
    tables (RoPE, sinusoidal, positions, embeddings)   at most 2^12 positions x 5120 floats = 80 MiB
    int64 token ops            B * T <= 2^24 tokens of 8 bytes = 128 MiB, 2^27 bytes
References and tolerances are the ops' own, imported: tests/_dense_gemm_ref.py, _ln_fold_ref.py, _contacts_ref.py,
_pair_head_ref.py, _frontend_ref.py, _sae_ref.py, _align_ref.py, _stream_edit_ref.py, and from the tests that hold them:
test_attention_variants_gpu.py (_ref, _check_ctx, _check_lse, _check_probs), test_precision_ops_gpu.py (ln64, LN_TOL,
gelu_x3_bound), test_f16x2_gpu.py (SPLIT_STORE_T_TOL, SPLIT_GELU_TOL), test_ln_fold_gpu.py (ROWSTATS_TOL),
test_round2_gpu.py (ROW_MEAN_TOL), test_kernels_gpu.py (contact_head_ref, CONTACTS_TOL).  The only new numbers are the
shapes, which tests/test_index_width_cpu.py checks.

MEASURED on an MI355X (`pytest -s` prints both figures per case): wall time, torch.cuda.max_memory_allocated()
    dense operand-dtype out, 4 kernels + bf16   0.03 - 0.79 s    7.18 GiB      fc1 of 15B            1.08 s   7.15 GiB
    dense fp32 out, 4 kernels                   0.04 - 0.06 s    6.41 GiB      residual, 8 GiB       1.03 s  10.44 GiB
    A operand                                   0.01 s           7.13 GiB      linear_split          0.09 s   7.18 GiB
    linear_gelu_x3                              0.13 s           7.22 GiB      attention d128        1.10 s  19.23 GiB
    attention d64 fp16 / bf16                   0.05 / 1.26 s   19.29 GiB      packed attention      0.14 s  20.79 GiB
    maps d64 / d128                             0.01 s           6.16 GiB      MSA column maps       1.51 s   5.39 GiB
    unfused contacts                            0.06 s           5.94 GiB      fused contacts + pair head   0.52 s  11.11 GiB
    q / k / v, 4 forms                          0.09 - 1.42 s   21.20 GiB      fold producer / consumer     0.03 / 0.02 s  8.84 / 7.16 GiB
    LayerNorm, 6 forms                          0.02 - 2.06 s   12.67 GiB      row kernels           0.19 s   8.13 GiB
    add_positions                               0.02 s           8.13 GiB
Every chunk of every case was bit-equal to the full run; the dense kernels' sampled rows lie at the same fraction of their
fp64 bound as in tests/test_dense_gemm_gpu.py (0.97 - 0.995 for the operand-dtype epilogues, 0.015 - 0.095 for the fp32
ones)."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import _dense_gemm_ref as D
import _index_width as W
from _ln_fold_ref import gelu64
from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu

BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
LOG2E = ops.LOG2E


def sentinel_of(dtype):
    return W.SENT32 if dtype == torch.float32 else W.SENT16


@pytest.fixture(autouse=True)
def _measure(request):
    """wall time and peak device memory of every case (`pytest -s`); memory is handed back afterwards"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[index width] {request.node.name}: {time.perf_counter() - t0:.2f} s, max_memory_allocated "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    N.check(N.lib.esmk_debug_gemm_impl(0, 0))
    torch.cuda.empty_cache()


def gate(case):
    reason = W.memory_gate(case.name, case.peak_bytes, torch.cuda.mem_get_info()[0])
    if reason:
        pytest.skip(reason)


def test_sentinels_are_those_of_the_precision_tests():
    import test_precision_ops_gpu as P

    assert P.SENT16 == W.SENT16
    buf = P.sent_buf(2, 4, torch.float32)
    assert bool((buf.view(torch.int32) == W.SENT32).all()) and P.untouched(buf)
    assert P.untouched(alloc_sentinel(3, (8,), torch.float16, guard=0)) and P.untouched(alloc_sentinel(3, (8,), torch.float32, guard=0))


# ---- slice-wise fill --------------------------------------------------------------------------------------------------
def slices(n, per_unit):
    step = max(1, W.MAX_ELEMS // per_unit)
    return [(s, min(n, s + step)) for s in range(0, n, step)]


def alloc_sentinel(units, unit_shape, dtype, guard=1):
    """[units + guard, *unit_shape] holding the sentinel, filled in slices below 2^30 elements"""
    buf = torch.empty((units + guard, *unit_shape), dtype=dtype, device="cuda")
    b = buf.view(BITS[dtype])
    for s0, s1 in slices(units + guard, math.prod(unit_shape)):
        b[s0:s1].fill_(sentinel_of(dtype))
    return buf


def rand_units(seed, u0, shape, dtype, scale=1.0, shift=0.0):
    """the i.i.d. random units [u0, u0 + shape[0]) of a tensor: a function of (seed, u0, shape), so a chunk can be made again"""
    g = torch.Generator(device="cuda").manual_seed(seed * 1_000_003 + u0)
    t = torch.randn(shape, device="cuda", generator=g)
    if scale != 1.0:
        t.mul_(scale)
    if shift != 0.0:
        t.add_(shift)
    return t.to(dtype)


def fill_random(t, chunks, seed, scale=1.0, shift=0.0):
    for u0, u1 in chunks:
        t[u0:u1].copy_(rand_units(seed, u0, (u1 - u0, *t.shape[1:]), t.dtype, scale, shift))


def pick(t, u0, units):
    """rows `units` of t, gathered from the slice [u0, ...) so that the index arithmetic of the gather stays small"""
    idx = torch.tensor([u - u0 for u in units], device="cuda")
    return t[u0:u0 + int(idx.max()) + 1][idx]


def samples_of(case):
    s = set()
    for t in case.tensors:
        s.update(W.sample_units(t.units, t.unit_bytes, t.boundaries()))
    return sorted(s)


def within(got, val, bound, what):
    frac = (got.double() - val).abs() / bound
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    worst = frac.max().item()
    assert worst <= 1.0, f"{what}: {worst:.2f} of the fp64 bound at flat index {frac.argmax().item()}; {int((frac > 1).sum())} elements fail"
    return worst


# ---- dense GEMM -------------------------------------------------------------------------------------------------------
# name -> (keywords of ops.linear, impl of esmk_debug_gemm_impl, flags of esmk_debug_gemm_plan, planned kernel)
KERNELS = {
    "auto": ({}, 0, 0, 9),
    "impl8": ({}, 8, 0, 8),
    "old": ({"force_old": True}, 0, 2, 256),
    "generic": ({"force_generic": True}, 0, 1, 64),
}
_T = (D.EPI_STORE_T, D.EPI_GELU_T)
_F = (D.EPI_STORE_F32, D.EPI_GELU_F32, D.EPI_RESID_F32)
FP16, BF16 = torch.float16, torch.bfloat16


def planned(M, Nn, K, epi, flags):
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, Nn, K, epi, flags, out))
    return out[0]


def weights(Nn, K, dtype, seed):
    """w and bias of _dense_gemm_ref.case: rows scaled by a linspace over N and by K^-1/2"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(Nn, K, device="cuda", generator=g) * (torch.linspace(0.5, 1.5, Nn, device="cuda") / math.sqrt(K))[:, None]).to(dtype)
    return w, torch.randn(Nn, device="cuda", generator=g)


def run_gemm(case, dtype, kernel, epilogues):
    gate(case)
    M, Nn, K = case.shape["M"], case.shape["N"], case.shape["K"]
    kw, impl, flags, want = KERNELS[kernel]
    N.check(N.lib.esmk_debug_gemm_impl(impl, 0))
    samples = samples_of(case)
    a = torch.empty((M, K), dtype=dtype, device="cuda")
    fill_random(a, W.chunk_list(M, K * 2), seed=11)
    w, bias = weights(Nn, K, dtype, seed=12)
    for epi in epilogues:
        got_kernel = planned(M, Nn, K, epi, flags)
        assert got_kernel == want, (kernel, got_kernel)
        odt = D.out_dtype(epi, dtype)
        chunks = W.chunk_list(M, max(Nn * odt.itemsize, K * 2))
        resid = epi == D.EPI_RESID_F32
        full = alloc_sentinel(M, (Nn,), odt)
        if resid:
            fill_random(full[:M], chunks, seed=13)
        ops.linear(a, w, bias, epi, out=full[:M], **kw)
        scratch = torch.empty((chunks[0][1], Nn), dtype=odt, device="cuda")

        def run_chunk(u0, u1):
            s = scratch[:u1 - u0]
            if resid:
                s.copy_(rand_units(13, u0, (u1 - u0, Nn), odt))
            ops.linear(a[u0:u1], w, bias, epi, out=s, **kw)
            return s.view(BITS[odt])

        worst = []

        def reference(u0, u1, units):
            r = pick(rand_units(13, u0, (u1 - u0, Nn), odt), 0, [u - u0 for u in units]) if resid else None
            val, bound = D.expected(epi, pick(a, u0, units), w, bias, r, generic=kernel == "generic")
            worst.append(within(pick(full, u0, units), val, bound, f"{case.name} {kernel} {D.EPI_NAMES[epi]} rows {units[0]}..{units[-1]}"))

        W.check_units(full.view(BITS[odt]), M, sentinel_of(odt), chunks, run_chunk, samples, reference, written=not resid,
                      what=f"{case.name} {kernel} {D.EPI_NAMES[epi]} {dtype}")
        print(f"\n{case.name} {kernel} {D.EPI_NAMES[epi]} {dtype}: kernel {got_kernel}, {len(chunks)} chunks bit-equal, "
              f"{len(samples)} sampled rows at {max(worst):.3f} of the fp64 bound")
        del full, scratch


@pytest.mark.parametrize("kernel,dtype", [("generic", FP16), ("old", FP16), ("impl8", FP16), ("auto", FP16), ("auto", BF16)],
                         ids=["generic-fp16", "old-fp16", "impl8-fp16", "auto-fp16", "auto-bf16"])
def test_dense_operand_dtype_out(kernel, dtype):
    """store_t and gelu_t: row 419,430 of the output holds byte 2^32 and element 2^31"""
    run_gemm(W.CASES["dense_t"], dtype, kernel, _T)


def test_fc1_of_15b():
    """rows of 40,960 bytes: 2^32 bytes at row 104,857"""
    run_gemm(W.CASES["fc1_15b"], FP16, "auto", (D.EPI_GELU_T,))


@pytest.mark.parametrize("kernel", ["generic", "old", "impl8", "auto"])
def test_dense_fp32_out(kernel):
    """store_f32, gelu_f32 and the residual epilogue (from a random `out`): 2^32 bytes at row 209,715"""
    run_gemm(W.CASES["dense_f32"], FP16, kernel, _F)


def test_residual_element_index():
    """8.0 GiB of fp32: the residual tile is read and written past element 2^31"""
    run_gemm(W.CASES["resid_elems"], FP16, "auto", (D.EPI_RESID_F32,))


def test_a_operand():
    """A rows of 5120 bytes, N = 64: the loads of row 838,860 and behind lie past 2^32 bytes"""
    run_gemm(W.CASES["a_operand"], FP16, "auto", (D.EPI_STORE_T,))


# ---- f16x2 / f16x3 ----------------------------------------------------------------------------------------------------
def test_linear_split():
    """ops.linear_split, store_t and gelu_t; (b) holds the sampled rows to the two figures of
    tests/test_f16x2_gpu.py::test_linear_split_matches_fp64 (SPLIT_STORE_T_TOL, SPLIT_GELU_TOL)"""
    from test_f16x2_gpu import SPLIT_GELU_TOL, SPLIT_STORE_T_TOL

    case = W.CASES["split_t"]
    gate(case)
    M, Nn, K = case.shape["M"], case.shape["N"], case.shape["K"]
    samples = samples_of(case)
    a = torch.empty((M, K), dtype=FP16, device="cuda")
    fill_random(a, W.chunk_list(M, K * 2), seed=21)
    g = torch.Generator(device="cuda").manual_seed(22)
    w = torch.randn(Nn, K, device="cuda", generator=g) / math.sqrt(K)
    bias = torch.randn(Nn, device="cuda", generator=g)
    w2 = ops.split_weight(w)
    chunks = W.chunk_list(M, Nn * 2)
    for epi in _T:
        assert planned(M, Nn, K, epi, 8) == 9  # flag 8: the GEMM over the [N, 2K] hi | lo image
        full = alloc_sentinel(M, (Nn,), FP16)
        ops.linear_split(a, w2, bias, epi, out=full[:M])
        scratch = torch.empty((chunks[0][1], Nn), dtype=FP16, device="cuda")

        def run_chunk(u0, u1):
            return ops.linear_split(a[u0:u1], w2, bias, epi, out=scratch[:u1 - u0]).view(torch.int16)

        def reference(u0, u1, units):
            ref = pick(a, u0, units).double() @ w.double().t() + bias.double()
            got = pick(full, u0, units).double()
            if epi == D.EPI_STORE_T:
                assert (got - ref).abs().max().item() / ref.abs().max().item() < SPLIT_STORE_T_TOL
            else:
                want = torch.nn.functional.gelu(ref)
                assert (got - want).abs().max().item() < SPLIT_GELU_TOL * want.abs().max().item()

        W.check_units(full.view(torch.int16), M, W.SENT16, chunks, run_chunk, samples, reference, what=f"linear_split {D.EPI_NAMES[epi]}")
        del full, scratch


def test_linear_gelu_x3():
    """ops.linear_gelu_x3: output rows of 3 N (hi | hi | lo); (b) is the bound of
    tests/test_precision_ops_gpu.py::test_linear_gelu_x3 on the sampled rows"""
    from test_precision_ops_gpu import gelu_x3_bound

    case = W.CASES["gelu_x3"]
    gate(case)
    M, Nn, K3 = case.shape["M"], case.shape["N"], case.shape["K"]
    K = K3 // 3
    samples = samples_of(case)
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.nn.functional.layer_norm(torch.randn(M, K, device="cuda", generator=g), (K,))
    a3 = torch.empty((M, K3), dtype=FP16, device="cuda")
    ops.layernorm_ex(x, torch.ones(K, device="cuda"), torch.zeros(K, device="cuda"), a3, None, x3=True)
    w = torch.randn(Nn, K, device="cuda", generator=g) / math.sqrt(K)
    w3 = torch.empty((Nn, K3), dtype=FP16, device="cuda")
    ops.split_weight_ex(w, w3, K, 3)
    bias = (torch.linspace(-8, 8, Nn, device="cuda") + 0.3 * torch.randn(Nn, device="cuda", generator=g))[torch.randperm(Nn, device="cuda", generator=g)]
    chunks = W.chunk_list(M, 3 * Nn * 2)
    full = alloc_sentinel(M, (3 * Nn,), FP16)
    assert planned(M, Nn, K3, D.EPI_GELU_T, 32) == 9  # flag 32: the hi | hi | lo output form
    ops.linear_gelu_x3(a3, w3, bias, full, M=M)
    scratch = torch.empty((chunks[0][1], 3 * Nn), dtype=FP16, device="cuda")

    def run_chunk(u0, u1):
        s = scratch[:u1 - u0]
        ops.linear_gelu_x3(a3[u0:u1], w3, bias, s, M=u1 - u0)
        return s.view(torch.int16)

    def reference(u0, u1, units):
        a3d, w3d = pick(a3, u0, units).double(), w3.double()
        pre = a3d @ w3d.t() + bias.double()
        t = pick(full, u0, units).view(len(units), Nn // 64, 3, 64)
        hi, hi2, lo = (t[:, :, s].reshape(len(units), Nn) for s in range(3))
        assert torch.equal(hi2.view(torch.int16), hi.view(torch.int16))
        v = hi.double() + lo.double()
        within(v, gelu64(pre), gelu_x3_bound(a3d, w3d, bias, pre, v, K), f"linear_gelu_x3 rows {units[0]}..{units[-1]}")

    W.check_units(full.view(torch.int16), M, W.SENT16, chunks, run_chunk, samples, reference, what="linear_gelu_x3")


# ---- attention ------------------------------------------------------------------------------------------------------------
def attention_into(q, k, vt, ctx, lse, key_bias=None, seq_info=None):
    """the launch of ops.attention into the caller's ctx [B*T, H*D] and lse [B,H,T] (log2 domain, as the kernel writes it)"""
    B, H, T, Dh = q.shape
    if seq_info is None and Dh == 64:
        N.check(N.lib.esmk_op_attention(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), N.ptr(ctx), N.ptr(lse), B, H, T,
                                        N.dtype_code(q.dtype), N.cur_stream()))
    else:
        N.check(N.lib.esmk_op_attention_ex(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), N.ptr(seq_info), None, N.ptr(ctx),
                                           N.ptr(lse), B, H, T, vt.shape[-1], Dh, 0, N.dtype_code(q.dtype), N.cur_stream()))


@pytest.mark.parametrize("name,dtype", [("attention_d128", FP16), ("attention_d64", FP16), ("attention_d64", BF16)],
                         ids=["d128-fp16", "d64-fp16", "d64-bf16"])
def test_attention(name, dtype):
    """q, k, v^T and ctx of 4.0 GiB each: (b, h) planes from 524,288 (head_dim 64) / 262,144 (128) on lie past 2^32 bytes.
    The units of the check are sequences b (H planes each; ctx rows b * T ..): the chunks are whole sequences."""
    from test_attention_variants_gpu import _check_ctx, _check_lse, _ref, _seq_info

    case = W.CASES[name]
    gate(case)
    B, H, T, Dh = (case.shape[x] for x in "BHTD")
    seq_bytes = H * T * Dh * 2
    chunks = W.chunk_list(B, seq_bytes)
    planes = samples_of(case)                         # (b, h) units
    seqs = sorted({p // H for p in planes})
    assert (W.B32 // (T * Dh * 2)) // H in seqs and B - 1 in seqs
    q = torch.empty((B, H, T, Dh), dtype=dtype, device="cuda")
    k = torch.empty_like(q)
    vt = torch.empty((B, H, Dh, T), dtype=dtype, device="cuda")
    fill_random(q, chunks, seed=41, scale=0.6 * LOG2E)    # the log2-domain operand of test_attention_variants_gpu._inputs
    fill_random(k, chunks, seed=42, scale=0.6 * math.sqrt(64.0 / Dh))
    fill_random(vt, chunks, seed=43)
    ctx = alloc_sentinel(B, (T, H * Dh), dtype)        # [B + 1, T, H * D]: the kernel's [B*T, H*D] and one guard sequence
    lse = alloc_sentinel(B, (H, T), torch.float32)
    attention_into(q, k, vt, ctx, lse)
    nb = chunks[0][1]
    ctx_s = torch.empty((nb, T, H * Dh), dtype=dtype, device="cuda")
    lse_s = torch.empty((nb, H, T), dtype=torch.float32, device="cuda")
    pos = ops.permute_keys16(T).cuda()

    def run_chunk(u0, u1):
        attention_into(q[u0:u1], k[u0:u1], vt[u0:u1], ctx_s[:u1 - u0], lse_s[:u1 - u0])
        return ctx_s[:u1 - u0].view(torch.int16), lse_s[:u1 - u0].view(torch.int32)

    def reference(u0, u1, units):
        qs, ks, vts = pick(q, u0, units), pick(k, u0, units), pick(vt, u0, units)
        v = vts[:, :, :, pos].transpose(2, 3)          # the inverse of ops.make_vt
        _, o_ref, lse_ref = _ref(qs.float() / LOG2E, ks, v)
        _check_ctx(pick(ctx, u0, units).reshape(len(units) * T, H * Dh), o_ref, dtype)
        _check_lse(pick(lse, u0, units) / LOG2E, lse_ref)

    W.check_units((ctx.view(torch.int16), lse.view(torch.int32)), B, (W.SENT16, W.SENT32), chunks, run_chunk, seqs, reference,
                  what=(f"{name} ctx", f"{name} lse"))

    # the padded form with seq_info on the LAST chunk's sequences, addressed inside the full tensors: trailing pads in
    # every third sequence; real rows are bit-equal to the plain run of the sequence cut to its length
    u0, u1 = chunks[-1]
    n = u1 - u0
    bias = torch.zeros((n, T), device="cuda")
    lens = [T if i % 3 else 1 + (7 * i) % (T - 1) for i in range(n)]
    for i, L in enumerate(lens):
        bias[i, L:] = float("-inf")
    info = _seq_info(bias)
    pctx = alloc_sentinel(n, (T, H * Dh), dtype)
    plse = alloc_sentinel(n, (H, T), torch.float32)
    attention_into(q[u0:u1], k[u0:u1], vt[u0:u1], pctx, plse, key_bias=bias, seq_info=info)
    assert bool((pctx[n:].view(torch.int16) == W.SENT16).all()) and bool((plse[n:].view(torch.int32) == W.SENT32).all())
    assert torch.isfinite(pctx[:n]).all() and torch.isfinite(plse[:n]).all()
    full_len = torch.tensor([L == T for L in lens], device="cuda")
    assert torch.equal(pctx[:n][full_len], ctx[u0:u1][full_len]) and torch.equal(plse[:n][full_len], lse[u0:u1][full_len])
    for i in [i for i, L in enumerate(lens) if L < T][-3:]:   # the padded sequences at the far end, each alone at its length
        L = lens[i]
        b = u0 + i
        v = vt[b:b + 1][:, :, :, pos].transpose(2, 3)[:, :, :L].contiguous()
        alone = ops.attention(q[b:b + 1, :, :L].contiguous(), k[b:b + 1, :, :L].contiguous(), ops.make_vt(v), want_lse=True)
        assert torch.equal(pctx[i, :L], alone[0]), (b, L)
        assert torch.equal(plse[i, :, :L] / LOG2E, alone[1][0]), (b, L)
    del q, k, vt, ctx, lse


# ---- token-packed attention --------------------------------------------------------------------------------------------------
def test_attention_packed():
    """esmk_op_attention_packed (what ops.attention_packed launches, into the caller's ctx) at H 40, head_dim 64, 839,232
    packed rows in 6556 segments of 128 and one of 64: q, k [H, rows, 64] pass 2^32 bytes in head 39, ctx [rows, 2560] at row
    838,860.  Chunks are runs of whole segments (copied out of the head-major tensors); the segments at the boundaries and at
    both ends are bit-equal to the segment alone through ops.attention and held to the fp64 softmax of
    tests/test_attention_variants_gpu.py, as tests/test_attention_packed_ops_gpu.py does at small sizes."""
    from test_attention_variants_gpu import _check_ctx, _check_lse, _ref

    case = W.CASES["attention_packed"]
    gate(case)
    H, rows, Dh = case.shape["H"], case.shape["rows"], case.shape["D"]
    segs = [(r, min(128, rows - r)) for r in range(0, rows, 128)]
    assert len(segs) == 6557 and segs[-1] == (rows - 64, 64)
    heads = W.chunk_list(H, (rows + 64) * 128)
    q = torch.empty((H, rows, Dh), dtype=FP16, device="cuda")
    k = torch.empty_like(q)
    vt = torch.empty((H, Dh, rows + 64), dtype=FP16, device="cuda")
    fill_random(q, heads, seed=141, scale=0.6 * LOG2E)
    fill_random(k, heads, seed=142, scale=0.6)
    fill_random(vt, heads, seed=143)
    for h in range(H):
        vt[h, :, rows:] = 0                                  # the spare key tile behind the last row
    ctx = alloc_sentinel(rows, (H * Dh,), FP16)
    lse = torch.empty((H, rows), device="cuda")

    def launch(q_, k_, vt_, segs_, n_rows, ctx_, lse_):
        seg, seg_ptr = ops._segments_arg(segs_)
        N.check(N.lib.esmk_op_attention_packed(N.ptr(q_), N.ptr(k_), N.ptr(vt_), None, seg_ptr, seg.shape[0], n_rows, vt_.shape[-1], H, Dh,
                                               N.dtype_code(FP16), None, None, N.ptr(ctx_), N.ptr(lse_), N.cur_stream()))

    launch(q, k, vt, segs, rows, ctx, lse)
    cb = ctx.view(torch.int16)
    assert bool((cb[rows:] == W.SENT16).all()), "store behind the last row"
    per = (W.CHUNK_BYTES - 1) // (H * 128) // 128 * 128      # rows of a chunk: whole segments, below 2^30 bytes per tensor
    for r0 in range(0, rows, per):
        r1 = min(rows, r0 + per)
        n = r1 - r0
        qc, kc = torch.empty((H, n, Dh), dtype=FP16, device="cuda"), torch.empty((H, n, Dh), dtype=FP16, device="cuda")
        vc = torch.zeros((H, Dh, n + 64), dtype=FP16, device="cuda")
        for h in range(H):                                   # head by head: every copy stays inside one head's slab
            qc[h], kc[h], vc[h, :, :n] = q[h, r0:r1], k[h, r0:r1], vt[h][:, r0:r1]
        cc = alloc_sentinel(n, (H * Dh,), FP16, guard=0)
        lc = torch.empty((H, n), device="cuda")
        launch(qc, kc, vc, [(a - r0, m) for a, m in segs if r0 <= a < r1], n, cc, lc)
        assert not bool((cb[r0:r1] == W.SENT16).any()), f"rows [{r0}, {r1}): unwritten element of ctx"
        assert torch.equal(cb[r0:r1], cc.view(torch.int16)), f"ctx rows [{r0}, {r1}) differ from the chunk run alone"
        assert torch.equal(lse[:, r0:r1].contiguous().view(torch.int32), lc.view(torch.int32)), f"lse rows [{r0}, {r1}) differ from the chunk"
        del qc, kc, vc, cc, lc
    at = lambda byte, unit: byte // unit                      # noqa: E731
    picks = {0, 1, len(segs) - 2, len(segs) - 1}
    for edge in (W.B31, W.B32):
        picks.add(at(edge, H * Dh * 2) // 128)                # the segment whose ctx rows hold the boundary
        picks.add((at(edge, 128) % rows) // 128)              # the segment whose q / k rows hold it (in head edge / 128 / rows)
    for i in sorted(picks):
        r0, n = segs[i]
        sl = slice(r0, r0 + n)
        pos = ops.permute_keys16(n).cuda()
        qs, ks = torch.stack([q[h, sl] for h in range(H)])[None], torch.stack([k[h, sl] for h in range(H)])[None]
        vs = torch.stack([vt[h][:, sl] for h in range(H)])[:, :, pos].transpose(1, 2)[None].contiguous()
        a_ctx, a_lse = ops.attention(qs, ks, ops.make_vt(vs), want_lse=True)
        assert torch.equal(ctx[sl], a_ctx) and torch.equal(lse[:, sl] / LOG2E, a_lse[0]), f"segment {i} differs from the segment alone"
        _, o_ref, lse_ref = _ref(qs.float() / LOG2E, ks, vs)
        _check_ctx(ctx[sl], o_ref, FP16)
        _check_lse((lse[:, sl] / LOG2E)[None], lse_ref)
    del q, k, vt, ctx


# ---- [B, L, H, T, T]: the padded attention maps and the unfused contact head ---------------------------------------------
def sequences_of(case):
    t = case.tensors[0]
    per = case.shape["L"] * case.shape["H"]
    return sorted({p // per for p in W.sample_units(t.units, t.unit_bytes, t.boundaries())})


@pytest.mark.parametrize("Dh", [64, 128])
def test_attention_maps_padded(Dh):
    """ops.attention_probs into layer 32 of a [26, 33, 20, 256, 256] fp32 tensor: the planes of sequences 24 and 25 lie past
    2^32 bytes.  The other 32 layers must keep the sentinel.  Units of the check: sequences."""
    from test_attention_variants_gpu import _check_probs, _inputs, _ref

    case = W.CASES["maps_padded"]
    gate(case)
    B, L, H, T = (case.shape[x] for x in "BLHT")
    layer = L - 1
    seqs = sequences_of(case)
    assert 24 in seqs and 25 in seqs and 0 in seqs
    qk, q, k, v = _inputs(ops, B, H, T, Dh, FP16, 0.6, seed=101)
    _, lse = ops.attention(qk, k, ops.make_vt(v), want_lse=True)
    chunks = W.chunk_list(B, L * H * T * T * 4)
    out = alloc_sentinel(B, (L, H, T, T), torch.float32)
    ops.attention_probs(qk, k, lse, out=out[:B], layer=layer, num_layers=L)
    scratch = torch.empty((chunks[0][1], L, H, T, T), device="cuda")

    def run_chunk(u0, u1):
        s = scratch[:u1 - u0]
        s.view(torch.int32).fill_(W.SENT32)
        ops.attention_probs(qk[u0:u1], k[u0:u1], lse[u0:u1].contiguous(), out=s, layer=layer, num_layers=L)
        return s.view(torch.int32)

    def reference(u0, u1, units):
        idx = torch.tensor(units, device="cuda")
        p_ref, _, _ = _ref(q[idx], k[idx], v[idx])
        _check_probs(pick(out, u0, units)[:, layer], p_ref, torch.float32)

    W.check_units(out.view(torch.int32), B, W.SENT32, chunks, run_chunk, seqs, reference, written=False, what=f"maps d{Dh}")
    ob = out.view(torch.int32)
    for b in range(B):
        assert bool((ob[b, :layer] == W.SENT32).all()), f"sequence {b}: a layer other than {layer} was written"
        assert not bool((ob[b, layer] == W.SENT32).any()), f"sequence {b}: unwritten element of layer {layer}"
    del out, scratch


def test_attention_maps_msa_columns():
    """ops.attention_probs(msa_C=513) into layer 11 of col_attentions [1, 12, 12, 513, 128, 128] fp32 (4.5 GiB): every plane
    of the written layer lies past 2^32 bytes.  The other 11 layers and the guard plane keep the sentinel; every column is
    bit-equal to the op on its half of the columns (one layer, so below 2^30 bytes); columns 0, 1, 256 and 512 are held to
    the fp64 fill-mode softmax of tests/test_attention_variants_gpu.py::test_msa_column_fill."""
    from test_attention_variants_gpu import _check_probs, _inputs, _ref

    case = W.CASES["maps_msa"]
    gate(case)
    L, H, C, R = (case.shape[x] for x in "LHCR")
    layer = L - 1
    assert ((layer * H) * C) * R * R * 4 >= W.B32
    qk, q, k, v = _inputs(ops, C, H, R, 64, FP16, 0.6, seed=151)
    flags = torch.zeros(C, R, device="cuda")
    flags[0, R // 2] = flags[0, R - 1] = 1.0
    flags[1::3, ::5] = 1.0
    flags[C - 1, :] = 1.0
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    _, lse = ops.attention(qk, k, ops.make_vt(v), flags, want_lse=True, fill_any_pad=one)
    n = L * H * C * R * R
    flat = torch.empty(n + R * R, device="cuda")
    fb = flat.view(torch.int32)
    for s0, s1 in slices(n + R * R, 1):
        fb[s0:s1].fill_(W.SENT32)
    out = flat[:n].view(1, L, H, C, R, R)
    ops.attention_probs(qk, k, lse, flags, out=out, layer=layer, num_layers=L, fill_any_pad=one, msa_C=C)
    ob = out.view(torch.int32)
    assert bool((fb[n:] == W.SENT32).all()), "store behind the last plane"
    for l in range(L):
        if l != layer:
            assert bool((ob[0, l] == W.SENT32).all()), f"layer {l} was written"
    for c0 in range(0, C, 257):
        c1 = min(C, c0 + 257)
        part = ops.attention_probs(qk[c0:c1], k[c0:c1], lse[c0:c1].contiguous(), flags[c0:c1].contiguous(), fill_any_pad=one, msa_C=c1 - c0)
        for h in range(H):
            got = ob[0, layer, h, c0:c1]
            assert not bool((got == W.SENT32).any()), f"head {h}, columns [{c0}, {c1}): unwritten element"
            assert torch.equal(got, part[0, 0, h].view(torch.int32)), f"head {h}, columns [{c0}, {c1}) differ from the chunk run alone"
        del part
    cols = torch.tensor([0, 1, 256, C - 1], device="cuda")
    p_ref, _, _ = _ref(q[cols], k[cols], v[cols], fill=flags[cols])
    got = torch.stack([out[0, layer, :, c] for c in cols.tolist()])
    _check_probs(got, p_ref, torch.float32)
    del out, flat


def test_contacts_unfused():
    """ops.contacts reading [26, 660, 256, 256] fp32 (4.2 GiB): the planes of sequences 24 and 25 lie past 2^32 bytes.  Every
    sequence is bit-equal to the op on its chunk of sequences; the sampled ones are held to contact_head_ref of
    tests/test_kernels_gpu.py, evaluated in fp64, within its CONTACTS_TOL.  The launch is that of ops.contacts, into the
    caller's output (sentinel, one guard sequence)."""
    from test_kernels_gpu import CONTACTS_TOL, contact_head_ref

    case = W.CASES["contacts"]
    gate(case)
    B, L, H, T = (case.shape[x] for x in "BLHT")
    seqs = sequences_of(case)
    chunks = W.chunk_list(B, L * H * T * T * 4)
    attn = torch.empty((B, L, H, T, T), device="cuda")
    for u0, u1 in chunks:  # positive i.i.d. entries of the size of a probability
        attn[u0:u1].copy_(rand_units(111, u0, (u1 - u0, L, H, T, T), torch.float32).abs_().mul_(1.0 / T))
    g = torch.Generator(device="cuda").manual_seed(112)
    tokens = torch.randint(4, 24, (B, T), device="cuda", generator=g)
    tokens[:, 0] = 0
    tokens[:, T - 1] = 2
    tokens[1::2, T - 10] = 2
    tokens[1::2, T - 9:] = 1
    w = torch.randn(1, L * H, device="cuda", generator=g)
    bias = torch.randn(1, device="cuda", generator=g)
    S = T - 2
    scratch = torch.empty((B * L * H * (S + 1),), device="cuda")

    def launch(attn_, tokens_, out_, n):
        N.check(N.lib.esmk_op_contacts(N.ptr(attn_), N.ptr(tokens_), N.ptr(w.reshape(-1)), N.ptr(bias), N.ptr(scratch), N.ptr(out_), n,
                                       L * H, T, 2, 1, 1, N.cur_stream()))

    out = alloc_sentinel(B, (S, S), torch.float32)
    launch(attn, tokens, out, B)
    outs = torch.empty((chunks[0][1], S, S), device="cuda")

    def run_chunk(u0, u1):
        launch(attn[u0:u1], tokens[u0:u1].contiguous(), outs[:u1 - u0], u1 - u0)
        return outs[:u1 - u0].view(torch.int32)

    def reference(u0, u1, units):
        for b in units:
            ref = contact_head_ref(attn[b:b + 1].double(), tokens[b:b + 1], w.double(), bias.double())
            assert (out[b:b + 1].double() - ref).abs().max().item() < CONTACTS_TOL, b

    W.check_units(out.view(torch.int32), B, W.SENT32, chunks, run_chunk, seqs, reference, what="contacts")
    del attn


# ---- stacked q, k [L, B, H, T, D]: the fused contact head and the pair head ------------------------------------------------
def test_contacts_fused_and_pair_head():
    """ops.contacts_fused (head_groups pinned to 4 in the full run and in the chunks) and ops.pair_head on q, k
    [33, 400, 20, 128, 64] of 4.0 GiB each: byte 2^32 falls in layer 32 at sequence 307, byte 2^31 in layer 16 at sequence
    153.  Every sequence is bit-equal to the op on its chunk of sequences (a sequence's map does not depend on its batch:
    tests/test_pair_head_ops_gpu.py, tests/test_contacts_fused_gpu.py); the sequences at the boundaries and at both ends are
    held to tests/_contacts_ref.py and tests/_pair_head_ref.py."""
    from _contacts_ref import check_against_ref as check_contacts
    from _contacts_ref import contact_ref
    from _pair_head_ref import check_against_ref as check_pair
    from _pair_head_ref import pair_head_ref

    case = W.CASES["contacts_fused"]
    gate(case)
    L, B, H, T = (case.shape[x] for x in "LBHT")
    G, S, n_sym, C_out = 4, T - 2, 4, 6
    plane = T * 64 * 2
    b31, b32 = (W.B31 // plane // H) % B, (W.B32 // plane // H) % B
    assert (b31, b32) == (153, 307) and W.B32 // plane // H // B == L - 1
    seqs = sorted({0, 1, b31, b31 + 1, b32, b32 + 1, B - 1})
    q = torch.empty((L, B, H, T, 64), dtype=FP16, device="cuda")
    k = torch.empty_like(q)
    layers = W.chunk_list(L, B * H * plane)
    fill_random(q, layers, seed=131, scale=0.6 * LOG2E)
    fill_random(k, layers, seed=132, scale=0.6)
    g = torch.Generator(device="cuda").manual_seed(133)
    tok = torch.randint(4, 24, (B, T), device="cuda", generator=g)
    tok[:, 0] = 0
    tok[:, T - 1] = 2
    tok[1::3, T - 20] = 2
    tok[1::3, T - 19:] = 1
    kb = torch.where(tok.eq(1), float("-inf"), 0.0).float().contiguous()
    w = torch.randn(L * H, device="cuda", generator=g)
    b = torch.randn(1, device="cuda", generator=g) * 0.3
    w2 = torch.randn(L * H, C_out, device="cuda", generator=g)
    bias2 = torch.randn(C_out, device="cuda", generator=g)
    # the natural-log row log-sum-exp in fp64, as the references form it (the kernels take fp32(lse * log2 e) of exactly this)
    lse = torch.empty((L, B, H, T), dtype=torch.float64, device="cuda")
    for l in range(L):
        for h0 in range(0, B, 100):
            sl = slice(h0, h0 + 100)
            sc = (q[l, sl].float() / LOG2E).double() @ k[l, sl].double().transpose(-1, -2) + kb[sl].double()[:, None, None, :]
            lse[l, sl] = torch.logsumexp(sc, dim=-1)
            del sc
    out = alloc_sentinel(B, (S, S), torch.float32)
    maps, used = ops.contacts_fused(q, k, lse, tok, w, b, key_bias=kb, head_groups=G, out=out.view(-1))
    assert bool((out.view(torch.int32)[B:] == W.SENT32).all()), "contacts_fused: store behind the last map"
    pair = ops.pair_head(q, k, lse, w2, bias2, n_sym=n_sym, key_bias=kb, tokens=tok)
    assert maps.shape == (B, S, S) and pair.shape == (B, S, S, C_out)
    for u0, u1 in W.chunk_list(B, L * H * plane):
        qc, kc, lc = q[:, u0:u1].contiguous(), k[:, u0:u1].contiguous(), lse[:, u0:u1].contiguous()
        m, used_c = ops.contacts_fused(qc, kc, lc, tok[u0:u1].contiguous(), w, b, key_bias=kb[u0:u1].contiguous(), head_groups=G)
        assert used_c == used
        assert torch.equal(maps[u0:u1].view(torch.int32), m.view(torch.int32)), f"contacts_fused: sequences [{u0}, {u1}) differ from the chunk"
        pc = ops.pair_head(qc, kc, lc, w2, bias2, n_sym=n_sym, key_bias=kb[u0:u1].contiguous(), tokens=tok[u0:u1].contiguous())
        assert torch.equal(pair[u0:u1].view(torch.int32), pc.view(torch.int32)), f"pair_head: sequences [{u0}, {u1}) differ from the chunk"
        del qc, kc, lc, m, pc
    for bq in seqs:
        sl = slice(bq, bq + 1)
        qe = q[:, sl].float() / LOG2E
        ref = contact_ref(qe, k[:, sl], tok[sl], w, b, key_bias=kb[sl])
        check_contacts(maps[sl], ref, f"sequence {bq}")
        pref = pair_head_ref(qe, k[:, sl], w2, bias2, n_sym, key_bias=kb[sl], tokens=tok[sl])
        check_pair(pair[sl], pref, where=f"sequence {bq}")
    del q, k


# ---- q / k (RoPE) and V^T epilogues ------------------------------------------------------------------------------------------
def qkv_knob(v):
    N.check(N.lib.esmk_debug_set(b"qkv_one_launch", ctypes.c_double(v)))


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "ln_fold"])
@pytest.mark.parametrize("one_launch", [0, 1], ids=["two_launches", "one_launch"])
def test_qkv_rope_epilogues(one_launch, fold):
    """esmk_op_qkv_rope2 / esmk_op_qkv_rope_ln (what tests/test_qkv_epilogues_gpu.py drives) at E 2560, H 40, T 1024, B 821:
    q, k [B,H,T,64] and V^T [B,H,64,T] pass 2^32 bytes in sequence 819.  The units of the check are sequences.  (b): the
    plain form is bit-equal to gemm8's untouched epilogue on the sampled sequences (test_plain_form_equals_gemm8_bit_for_bit).
    The fold form runs as test_fold_form_is_gemm8_times_a_power_of_two_row_scale does: zero bias, ln_rstd[m] = 2^k(m), scaled
    operands, so q, k and V^T are gemm8's plain result times 2^k(row) bit for bit (fp16-subnormal elements within 2^-22), and
    V is also held to the fp64 bound of test_fold_form_with_bias_and_bias2_same_bits_in_every_launch_form.
    NOT COVERED: head_dim 128.  The single-op entries refuse head_dim != 64, and in the 15B-dims engine test q, k and V^T are
    1.09 GB each, below 2^31 bytes: the head_dim-128 q / k / v epilogues cross no boundary in any test."""
    case = W.CASES["qkv_rope"]
    gate(case)
    B, H, T, E = (case.shape[x] for x in "BHTE")
    dtype = FP16
    seqs = sorted({p // H for p in samples_of(case)})
    assert (W.B32 // (T * 64 * 2)) // H == 819 and 819 in seqs and B - 1 in seqs
    chunks = W.chunk_list(B, T * E * 2)
    qkv = ops.QkvHandle(E, H, operand_dtype=dtype)
    a = torch.empty((B, T, E), dtype=dtype, device="cuda")
    fill_random(a, chunks, seed=61)
    g = torch.Generator(device="cuda").manual_seed(62)
    w = (torch.randn(3 * E, E, device="cuda", generator=g) * ((1024.0 if fold else 1.0) / math.sqrt(E))).to(dtype)
    bias = torch.zeros(3 * E, device="cuda") if fold else 0.1 * torch.randn(3 * E, device="cuda", generator=g)
    bias2 = None
    rstd = None
    if fold:  # one per row, readable up to the next multiple of 256 rows (B * T is one): 2^-2 .. 2^2
        rstd = torch.exp2(((torch.arange(B * T, device="cuda") % 5) - 2).float())

    def launch(a_, rstd_, q_, k_, vt_, n):
        if fold:
            N.check(N.lib.esmk_op_qkv_rope_ln(qkv.h, N.ptr(a_), N.ptr(w), N.ptr(bias), N.ptr(bias2), N.ptr(rstd_), N.ptr(q_), N.ptr(k_),
                                              N.ptr(vt_), n, T, 1, N.cur_stream()))
        else:
            N.check(N.lib.esmk_op_qkv_rope2(qkv.h, N.ptr(a_), N.ptr(w), N.ptr(bias), N.ptr(q_), N.ptr(k_), N.ptr(vt_), n, T, 1,
                                            N.cur_stream()))

    q = alloc_sentinel(B, (H, T, 64), dtype)
    k = alloc_sentinel(B, (H, T, 64), dtype)
    vt = alloc_sentinel(B, (H, 64, T), dtype)
    nb = chunks[0][1]
    qs, ks, vts = (torch.empty((nb, *t.shape[1:]), dtype=dtype, device="cuda") for t in (q, k, vt))
    try:
        qkv_knob(one_launch)
        launch(a, rstd, q, k, vt, B)

        def run_chunk(u0, u1):
            n = u1 - u0
            launch(a[u0:u1], rstd[u0 * T:] if fold else None, qs[:n], ks[:n], vts[:n], n)
            return tuple(t[:n].view(torch.int16) for t in (qs, ks, vts))

        def reference(u0, u1, units):
            n = len(units)
            a_s = pick(a, u0, units).contiguous()
            if not fold:
                N.check(N.lib.esmk_debug_gemm_impl(8, 0))
                qkv_knob(-1)
                try:
                    launch(a_s, None, qs[:n], ks[:n], vts[:n], n)
                finally:
                    N.check(N.lib.esmk_debug_gemm_impl(0, 0))
                    qkv_knob(one_launch)
                for name, full, ref in (("q", q, qs), ("k", k, ks), ("vt", vt, vts)):
                    assert torch.equal(pick(full, u0, units), ref[:n]), f"{name} differs from gemm8's epilogue"
                return
            N.check(N.lib.esmk_debug_gemm_impl(8, 0))
            qkv_knob(-1)
            try:
                N.check(N.lib.esmk_op_qkv_rope2(qkv.h, N.ptr(a_s), N.ptr(w), N.ptr(bias), N.ptr(qs[:n]), N.ptr(ks[:n]), N.ptr(vts[:n]),
                                                n, T, 1, N.cur_stream()))
            finally:
                N.check(N.lib.esmk_debug_gemm_impl(0, 0))
                qkv_knob(one_launch)
            r_seq = torch.stack([rstd[u * T:(u + 1) * T] for u in units])          # [n, T]
            pos = ops.permute_keys16(T).cuda()                                      # V^T column pos[t] holds key t
            for name, full, ref, sc in (("q", q, qs, r_seq[:, None, :, None]), ("k", k, ks, r_seq[:, None, :, None]),
                                        ("vt", vt, vts, r_seq[:, None, None, :])):
                y, r = pick(full, u0, units), ref[:n].float()
                if name == "vt":
                    y, r = y[..., pos], r[..., pos]
                x = r * sc
                assert x.abs().max().item() <= 65504.0, name
                normal = (r.abs() >= 2.0 ** -14) & (x.abs() >= 2.0 ** -14) | (r == 0)
                assert (~normal).float().mean().item() < 1e-4, name
                assert torch.equal(x.to(dtype)[normal], y[normal]), f"{name} is not gemm8's result times the row's power of two"
                if (~normal).any():
                    assert (x - y.float())[~normal].abs().max().item() <= 2.0 ** -22, name
            rows = a_s.view(n * T, E)[::16]
            r64 = r_seq.reshape(-1)[::16].double()[:, None]
            v64 = (rows.double() @ w[2 * E:].double().t()) * r64
            mag = (rows.double().abs() @ w[2 * E:].double().abs().t()) * r64
            got = pick(vt, u0, units)[..., pos].permute(0, 3, 1, 2).reshape(n * T, E)[::16].double()  # [n,H,64,T] -> [n*T, E]
            eps = 2.0 ** -11
            excess = (got - v64).abs() - (eps * v64.abs() + (E + 2) * 2.0 ** -24 * mag * (1 + eps))
            assert (excess <= 0).all(), float(excess.max())

        W.check_units(tuple(t.view(torch.int16) for t in (q, k, vt)), B, (W.SENT16,) * 3, chunks, run_chunk, seqs, reference,
                      what=("q", "k", "vt"))
    finally:
        qkv_knob(-1)
    del a, q, k, vt, qs, ks, vts


# ---- LayerNorm fold: producer and consumer epilogues ---------------------------------------------------------------------------
def linear_ln(a, w, bias, bias2, out, epilogue, M, rstd=None, h16=None, part=None, parts=0, mean=None):
    """esmk_op_linear_ln as tests/test_ln_fold_ops_gpu.py calls it (the library's choice of tile height)"""
    import _ln_fold_ref as R

    Nn, K = w.shape
    assert planned(M, Nn, K, epilogue, 4) == 9
    N.check(N.lib.esmk_op_linear_ln(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(bias2), N.ptr(out), M, Nn, K, epilogue, R.DT_CODE[a.dtype],
                                    N.ptr(rstd), N.ptr(h16), h16.shape[1] if h16 is not None else 0, N.ptr(part), parts, N.ptr(mean),
                                    0, N.cur_stream()))


def test_ln_fold_producer():
    """epilogue 4 of ops.linear_ln at M 419,800 x N 2560: out fp32 passes 2^32 bytes at row 419,430, h16 (rows of 2624
    fp16) 2^31 bytes at row 409,200; ln_part [M, 21, 2] is indexed by the row.  (b): tests/_ln_fold_ref.py producer and
    producer_side, as tests/test_ln_fold_ops_gpu.py::test_producer applies them."""
    import _ln_fold_ref as R

    case = W.CASES["ln_producer"]
    gate(case)
    M, Nn, K = case.shape["M"], case.shape["N"], case.shape["K"]
    P, ldh = (Nn + 127) // 128, (Nn + 63) // 64 * 64 + 64
    samples = samples_of(case)
    chunks = W.chunk_list(M, Nn * 4)
    a = torch.empty((M, K), dtype=FP16, device="cuda")
    fill_random(a, W.chunk_list(M, K * 2), seed=81)
    g = torch.Generator(device="cuda").manual_seed(82)
    w = (torch.randn(Nn, K, device="cuda", generator=g) / math.sqrt(K)).to(FP16)
    bias = torch.randn(Nn, device="cuda", generator=g)
    mean = torch.zeros(M + 512, device="cuda")          # readable up to the next multiple of 256 rows behind any chunk
    mean[:M] = 0.1 * torch.randn(M, device="cuda", generator=g)
    out = alloc_sentinel(M, (Nn,), torch.float32)
    fill_random(out[:M], chunks, seed=83)
    h16 = alloc_sentinel(M, (ldh,), FP16)
    part = alloc_sentinel(M, (P + 1, 2), torch.float32)  # one spare slab per row, which must stay as it is
    linear_ln(a, w, bias, None, out, D.EPI_RESID_F32, M, h16=h16, part=part, parts=P + 1, mean=mean)
    nb = chunks[0][1]
    outs = torch.empty((nb, Nn), device="cuda")
    hs = torch.empty((nb, ldh), dtype=FP16, device="cuda")
    ps = torch.empty((nb, P + 1, 2), device="cuda")

    def run_chunk(u0, u1):
        n = u1 - u0
        outs[:n].copy_(rand_units(83, u0, (n, Nn), torch.float32))
        hs[:n].view(torch.int16).fill_(W.SENT16)
        ps[:n].view(torch.int32).fill_(W.SENT32)
        linear_ln(a[u0:u1], w, bias, None, outs[:n], D.EPI_RESID_F32, n, h16=hs[:n], part=ps[:n], parts=P + 1, mean=mean[u0:])
        return outs[:n].view(torch.int32), hs[:n].view(torch.int16), ps[:n].view(torch.int32)

    def reference(u0, u1, units):
        loc = [u - u0 for u in units]
        x0 = pick(rand_units(83, u0, (u1 - u0, Nn), torch.float32), 0, loc)
        o = pick(out, u0, units)
        ref, bound = R.producer(pick(a, u0, units), w, bias, x0)
        within(o, ref, bound, f"producer out rows {units[0]}..{units[-1]}")
        _, h_ref, p_ref, p_bound = R.producer_side(o, pick(mean, u0, units), FP16)
        assert torch.equal(pick(h16, u0, units)[:, :Nn], h_ref), "h16 is not fp16(out - mean_prev)"
        err = (pick(part, u0, units)[:, :P].double() - p_ref).abs()
        assert bool((err <= p_bound).all()), "partial sums outside their bound"

    W.check_units((out.view(torch.int32), h16.view(torch.int16), part.view(torch.int32)), M, (W.SENT32, W.SENT16, W.SENT32), chunks,
                  run_chunk, samples, reference, written=False, what=("producer out", "producer h16", "producer ln_part"))
    hb, pb = h16.view(torch.int16), part.view(torch.int32)
    for s0, s1 in slices(M, ldh):
        assert not bool((hb[s0:s1, :Nn] == W.SENT16).any()), f"h16 rows [{s0}, {s1}): unwritten element"
        assert bool((hb[s0:s1, Nn:] == W.SENT16).all()), f"h16 rows [{s0}, {s1}): store past column N"
    assert not bool((pb[:M, :P] == W.SENT32).any()) and bool((pb[:M, P:] == W.SENT32).all()), "ln_part: unwritten slab or stray store"
    del out, h16, part, outs, hs, ps


def test_ln_fold_consumer():
    """epilogue 2 of ops.linear_ln (fc1 with the row's rstd) at M 210,000 x N 10240: out passes 2^32 bytes at row 209,715,
    ln_rstd is indexed by the row.  (b): tests/_ln_fold_ref.py consumer and gelu_out_bound (test_consumer)."""
    import _ln_fold_ref as R

    case = W.CASES["ln_consumer"]
    gate(case)
    M, Nn, K = case.shape["M"], case.shape["N"], case.shape["K"]
    samples = samples_of(case)
    chunks = W.chunk_list(M, Nn * 2)
    a = torch.empty((M, K), dtype=FP16, device="cuda")
    fill_random(a, W.chunk_list(M, K * 2), seed=91)
    g = torch.Generator(device="cuda").manual_seed(92)
    w = (torch.randn(Nn, K, device="cuda", generator=g) / math.sqrt(K)).to(FP16)
    bias, bias2 = torch.randn(Nn, device="cuda", generator=g), torch.randn(Nn, device="cuda", generator=g)
    rstd = torch.ones(M + 512, device="cuda")            # readable up to the next multiple of 256 rows behind any chunk
    rstd[:M] = 0.05 * (300 / 0.05) ** torch.rand(M, device="cuda", generator=g)
    out = alloc_sentinel(M, (Nn,), FP16)
    linear_ln(a, w, bias, bias2, out, D.EPI_GELU_T, M, rstd=rstd)
    scratch = torch.empty((chunks[0][1], Nn), dtype=FP16, device="cuda")

    def run_chunk(u0, u1):
        linear_ln(a[u0:u1], w, bias, bias2, scratch[:u1 - u0], D.EPI_GELU_T, u1 - u0, rstd=rstd[u0:])
        return scratch[:u1 - u0].view(torch.int16)

    def reference(u0, u1, units):
        pre, pre_bound = R.consumer(pick(a, u0, units), w, bias, bias2, pick(rstd, u0, units))
        val, bound = R.gelu_out_bound(pre, pre_bound, FP16)
        within(pick(out, u0, units), val, bound, f"consumer rows {units[0]}..{units[-1]}")

    W.check_units(out.view(torch.int16), M, W.SENT16, chunks, run_chunk, samples, reference, what="consumer out")
    del out, scratch


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, 0], ids=["engine_form", "variant0"])
@pytest.mark.parametrize("entry,ldy_pad,dtype", [("layernorm", 0, FP16), ("layernorm_ex", 0, BF16), ("layernorm_ex", 64, FP16)],
                         ids=["op-fp16", "ex-bf16", "ex-ldy-fp16"])
def test_layernorm(entry, ldy_pad, dtype, variant):
    """210,000 rows x 5120: x and y32 cross 2^32 bytes at row 209,715, y 2^31 bytes at the same row (ldy = E + 64: at row
    207,126).  y32 within LN_TOL of fp64, y == y32 rounded once (tests/test_precision_ops_gpu.py), columns past E untouched."""
    from test_precision_ops_gpu import LN_TOL, ln64

    case = W.CASES["layernorm"]
    gate(case)
    rows, E = case.shape["rows"], case.shape["E"]
    ldy = E + ldy_pad
    samples = samples_of(case)
    chunks = W.chunk_list(rows, E * 4)
    x = torch.empty((rows, E), device="cuda")
    fill_random(x, chunks, seed=51, scale=3.0, shift=0.5)
    g = torch.Generator(device="cuda").manual_seed(52)
    gamma = 1 + 0.1 * torch.randn(E, device="cuda", generator=g)
    beta = 0.1 * torch.randn(E, device="cuda", generator=g)
    y = alloc_sentinel(rows, (ldy,), dtype)
    y32 = alloc_sentinel(rows, (E,), torch.float32)
    code = N.dtype_code(dtype) | (0 if variant is None else (variant + 1) << 8)

    def launch(xs, ys, y32s):
        if entry == "layernorm":  # what ops.layernorm calls, into the caller's buffers
            N.check(N.lib.esmk_op_layernorm(N.ptr(xs), N.ptr(gamma), N.ptr(beta), N.ptr(ys), N.ptr(y32s), xs.shape[0], E, code,
                                            N.cur_stream()))
        else:
            ops.layernorm_ex(xs, gamma, beta, ys, y32s, operand_dtype=dtype, variant=variant)

    launch(x, y, y32)
    nb = chunks[0][1]
    ys = torch.empty((nb, ldy), dtype=dtype, device="cuda")
    y32s = torch.empty((nb, E), device="cuda")

    def run_chunk(u0, u1):
        ys[:u1 - u0].view(torch.int16).fill_(W.SENT16)  # the columns past E compare equal only if neither run wrote them
        launch(x[u0:u1], ys[:u1 - u0], y32s[:u1 - u0])
        return y32s[:u1 - u0].view(torch.int32), ys[:u1 - u0].view(torch.int16)

    def reference(u0, u1, units):
        o = pick(y32, u0, units)
        err = (o.double() - ln64(pick(x, u0, units), gamma, beta, 1e-5)).abs().max().item()
        assert err < LN_TOL, err
        assert torch.equal(pick(y, u0, units)[:, :E].view(torch.int16), o.to(dtype).view(torch.int16))

    W.check_units((y32.view(torch.int32), y.view(torch.int16)), rows, (W.SENT32, W.SENT16), chunks, run_chunk, samples, reference,
                  written=(True, ldy == E), what=(f"{entry} y32", f"{entry} y"))
    if ldy > E:  # nothing unwritten in the first E columns, nothing written behind them
        yb = y.view(torch.int16)
        for s0, s1 in slices(rows, ldy):
            assert not bool((yb[s0:s1, :E] == W.SENT16).any()), f"y rows [{s0}, {s1}): unwritten element"
            assert bool((yb[s0:s1, E:] == W.SENT16).all()), f"y rows [{s0}, {s1}): store past column E"
    del x, y, y32


# ---- the other row kernels of the layer loop ---------------------------------------------------------------------------------
def test_row_kernels():
    """One fp32 buffer of 210,000 rows x 5120 (2^32 bytes at row 209,715; B 210 x T 1000 where rows map to (b, t)), reused by
    embed, scale_rows, zero_gap_rows, rowstats, gather_rows, blend_rows, pool_rows and masked_row_mean.  The exact ops (a gather, one fp32
    product, zeros) are compared bit for bit with torch on every chunk, which is (a) and (b) at once; rowstats and
    masked_row_mean use the figures of tests/test_ln_fold_gpu.py::test_rowstats_against_torch and
    tests/test_round2_gpu.py::test_masked_row_mean_matches_torch."""
    import _align_ref as A
    import _frontend_ref as R
    import _sae_ref as S
    import _stream_edit_ref as SE
    from test_ln_fold_gpu import ROWSTATS_TOL
    from test_round2_gpu import ROW_MEAN_TOL

    case = W.CASES["row_kernels"]
    gate(case)
    rows, E = case.shape["rows"], case.shape["E"]
    B, T = 210, 1000
    assert B * T == rows
    samples = samples_of(case)
    chunks = W.chunk_list(rows, E * 4, multiple=T)       # whole sequences
    x = alloc_sentinel(rows, (E,), torch.float32)
    xb = x.view(torch.int32)
    g = torch.Generator(device="cuda").manual_seed(71)

    def guard_ok(what):
        assert bool((xb[rows:] == W.SENT32).all()), f"{what}: store behind the last row"

    # embed: tokens with <mask> and <pad>, one scale per sequence (distinct: a row read from another sequence differs)
    tokens = torch.randint(4, 24, (B, T), device="cuda", generator=g)
    tokens[:, 0] = 0
    tokens[:, 7] = 32
    tokens[::3, 900:] = 1
    table = torch.randn(33, E, device="cuda", generator=g)
    # powers of two: x * fp32(0.88) / scale has the same bits however the division is done; the cycle of 8 gives sequence b
    # and the sequences 2^31 and 2^32 bytes away (105 and 210 sequences) different scales
    scale = torch.exp2((torch.arange(B, device="cuda") % 8 - 4).float())
    ops.embed(tokens, table, scale, out=x[:rows].view(B, T, E))
    guard_ok("embed")
    for u0, u1 in chunks:
        b0, b1 = u0 // T, u1 // T
        want = R.embed_ref(tokens[b0:b1], table, scale[b0:b1]).view(u1 - u0, E)
        assert torch.equal(xb[u0:u1], want.view(torch.int32)), f"embed: rows [{u0}, {u1}) differ from the reference"
    print("\nrow kernels: embed bit-equal on every row")

    # scale_rows in place on i.i.d. rows
    fill_random(x[:rows], chunks, seed=72)
    keep = torch.where(torch.rand(rows, device="cuda", generator=g) < 0.1, 0.0, 1.0) * (0.5 + torch.rand(rows, device="cuda", generator=g))
    ops.scale_rows(x[:rows], keep)
    guard_ok("scale_rows")
    for u0, u1 in chunks:
        want = rand_units(72, u0, (u1 - u0, E), torch.float32) * keep[u0:u1, None]
        assert torch.equal(xb[u0:u1], want.view(torch.int32)), f"scale_rows: rows [{u0}, {u1}) differ from x * keep"
    print("row kernels: scale_rows bit-equal on every row")

    # zero_gap_rows clears the rows behind each segment: gaps across both boundary rows and behind the last segment.  The entry
    # takes a row count that is a multiple of 64 and segment starts that are multiples of 16; the rows behind rows_z stay.
    edge31, edge32 = W.B31 // (E * 4), W.B32 // (E * 4)
    rows_z = rows // 64 * 64
    s31, s32 = (edge31 // 16 + 1) * 16, (edge32 // 16 + 1) * 16
    segs = [(0, 1000), (2000, edge31 - 2000 - 3), (s31, edge32 - s31 - 7), (s32, rows_z - s32 - 40)]
    assert all(n > 0 for _, n in segs) and segs[-1][0] + segs[-1][1] < rows_z
    fill_random(x[:rows], chunks, seed=73)
    ops.zero_gap_rows(x, segs, rows_z, E * 4)
    guard_ok("zero_gap_rows")
    gap = R.gap_rows(segs, rows).cuda()
    gap[rows_z:] = False
    assert bool(gap[edge31]) and bool(gap[edge32]) and bool(gap[rows_z - 1]) and not bool(gap[s32]) and not bool(gap[rows - 1])
    for u0, u1 in chunks:
        want = rand_units(73, u0, (u1 - u0, E), torch.float32).masked_fill(gap[u0:u1, None], 0.0)
        assert torch.equal(xb[u0:u1], want.view(torch.int32)), f"zero_gap_rows: rows [{u0}, {u1}) differ"
    print("row kernels: zero_gap_rows bit-equal on every row")

    # rowstats: y = fp16(x - mean) [rows, E] (2^31 bytes at row 209,715), mean and rstd per row
    fill_random(x[:rows], chunks, seed=74, scale=2.0, shift=0.5)
    y = alloc_sentinel(rows, (E,), FP16)
    mean = alloc_sentinel(rows, (), torch.float32)
    rstd = alloc_sentinel(rows, (), torch.float32)

    def rowstats(xs, ys, ms, rs):
        N.check(N.lib.esmk_op_rowstats(N.ptr(xs), N.ptr(ys), N.ptr(ms), N.ptr(rs), xs.shape[0], E, E, N.dtype_code(FP16), N.cur_stream()))

    rowstats(x[:rows], y, mean, rstd)
    nb = chunks[0][1]
    ys = torch.empty((nb, E), dtype=FP16, device="cuda")
    ms, rs = torch.empty(nb, device="cuda"), torch.empty(nb, device="cuda")

    def run_chunk(u0, u1):
        n = u1 - u0
        rowstats(x[u0:u1], ys[:n], ms[:n], rs[:n])
        return ys[:n].view(torch.int16), ms[:n].view(torch.int32), rs[:n].view(torch.int32)

    def reference(u0, u1, units):
        xs = pick(x, u0, units)
        m, v = xs.double().mean(-1), xs.double().var(-1, unbiased=False)
        assert (pick(mean, u0, units).double() - m).abs().max().item() < ROWSTATS_TOL
        assert ((pick(rstd, u0, units).double() - torch.rsqrt(v + 1e-5)).abs() / torch.rsqrt(v + 1e-5)).max().item() < ROWSTATS_TOL
        assert torch.equal(pick(y, u0, units), (xs - pick(mean, u0, units)[:, None]).half())

    W.check_units((y.view(torch.int16), mean.view(torch.int32), rstd.view(torch.int32)), rows, (W.SENT16, W.SENT32, W.SENT32), chunks,
                  run_chunk, samples, reference, what=("rowstats y", "rowstats mean", "rowstats rstd"))
    guard_ok("rowstats")
    del y, ys
    print("row kernels: rowstats bit-equal to the chunks on every row")

    # gather_rows: sel on both sides of both boundaries, clamped ends
    sel = [0, 1, edge31 - 1, edge31, edge31 + 1, edge32 - 1, edge32, edge32 + 1, rows - 1, rows + 5, -3]
    out = alloc_sentinel(len(sel), (E,), torch.float32)
    ops.gather_rows(x[:rows], torch.tensor(sel, dtype=torch.int32, device="cuda"), out=out[:len(sel)])
    assert bool((out.view(torch.int32)[len(sel):] == W.SENT32).all())
    for i, r in enumerate(sel):
        r = min(max(r, 0), rows - 1)
        assert torch.equal(out[i].view(torch.int32), xb[r:r + 1][0]), f"gather_rows: sel {sel[i]} does not return row {r}"
    print("row kernels: gather_rows returns the rows on both sides of the boundaries")

    # blend_rows and pool_rows (big input, small output): lists of one entry return the source row exactly (blend: "a list
    # of one entry copies the row"; pool: an fp64 sum of one fp32 value), the sources on both sides of both boundaries
    src = [r for r in sel if 0 <= r < rows]
    src_t = torch.tensor(src, dtype=torch.int32, device="cuda")
    one = torch.arange(len(src) + 1, dtype=torch.int32, device="cuda")
    blend = ops.blend_rows(x[:rows], one, src_t, torch.ones(len(src), device="cuda"))
    pool = ops.pool_rows(x[:rows], src_t, one)
    for i, r in enumerate(src):
        assert torch.equal(blend[i].view(torch.int32), xb[r:r + 1][0]), f"blend_rows: source row {r}"
        assert torch.equal(pool[i].view(torch.int32), xb[r:r + 1][0]), f"pool_rows: source row {r}"
    print("row kernels: blend_rows and pool_rows read the rows on both sides of the boundaries")

    # sae_rows and align_rows: the f16x3 images of listed rows, bit for bit against tests/_sae_ref.py and tests/_align_ref.py
    x_src = torch.stack([x[r] for r in src]).cpu().numpy()
    b_dec = torch.randn(E, device="cuda", generator=g)
    img = alloc_sentinel(len(src), (3 * E,), FP16)
    ops.sae_rows(x[:rows], src_t, b_dec, 0.37, out=img, n=len(src))
    want = S.image_rows(S.u_rows(x_src, None, b_dec.cpu().numpy(), 0.37)).view(np.int16)
    got = img.view(torch.int16).cpu().numpy()
    assert np.array_equal(got[:len(src)], want) and (got[len(src):] == W.SENT16).all(), "sae_rows: image of the listed rows"
    for b_side in (False, True):
        img = alloc_sentinel(len(src), (3 * E,), FP16)
        ops.align_rows(x[:rows], src_t, cosine=True, b_side=b_side, out=img, n=len(src))
        want = A.image(A.operand_rows(x_src), b_side).view(np.int16)
        got = img.view(torch.int16).cpu().numpy()
        assert np.array_equal(got[:len(src)], want) and (got[len(src):] == W.SENT16).all(), f"align_rows b_side={b_side}"
    print("row kernels: sae_rows and align_rows image the rows on both sides of the boundaries")

    # masked_row_mean over [B, T, E]: sequences 0, 1, around both boundaries and the last
    counts = torch.randint(1, T - 1, (B,), device="cuda", generator=g, dtype=torch.int32)
    counts[B - 1] = T + 5
    out = ops.masked_row_mean(x[:rows].view(B, T, E), counts, first_row=1)
    x3 = x[:rows].view(B, T, E)
    for b in sorted({0, 1, edge31 // T - 1, edge31 // T, edge32 // T - 1, edge32 // T, B - 1}):
        want = x3[b, 1:int(counts[b]) + 1].double().mean(0)
        assert (out[b].double() - want).abs().max().item() < ROW_MEAN_TOL * max(1.0, T / 64), b
    for c0 in range(0, B, 50):  # every sequence: the op again on a chunk of sequences, bit for bit
        c1 = min(B, c0 + 50)
        again = ops.masked_row_mean(x3[c0:c1], counts[c0:c1].contiguous(), first_row=1)
        assert torch.equal(out[c0:c1], again), f"masked_row_mean: sequences [{c0}, {c1}) differ from the chunk run alone"
    print("row kernels: masked_row_mean bit-equal to the chunks on every sequence")

    # stream_edit (x' = keep x + gain s, in place) on listed rows on both sides of the boundaries, with the LayerNorm-fold
    # state of the edited rows (y fp16 [rows, E]: 2^31 bytes at row 209,715): x' against tests/_stream_edit_ref.py, y / mean /
    # rstd against rowstats of x', every other row of x, y, mean and rstd untouched
    vec = torch.randn(E, device="cuda", generator=g)
    y = alloc_sentinel(rows, (E,), FP16)
    mean = alloc_sentinel(rows, (), torch.float32)
    rstd = alloc_sentinel(rows, (), torch.float32)
    ops.stream_edit(x[:rows], SE.AXPBY, 0.5, 1.5, rows=src_t, src=vec, y=y, mean=mean, rstd=rstd)
    guard_ok("stream_edit")
    after = torch.stack([x[r] for r in src])
    want = SE.axpby_rows(x_src, vec.cpu().numpy()[None, :], 0.5, 1.5)
    assert np.array_equal(after.cpu().numpy().view(np.int32), want.view(np.int32)), "stream_edit: the edited rows"
    ys = torch.empty((len(src), E), dtype=FP16, device="cuda")
    ms, rs = torch.empty(len(src), device="cuda"), torch.empty(len(src), device="cuda")
    rowstats(after, ys, ms, rs)
    edited = torch.zeros(rows + 1, dtype=torch.bool, device="cuda")
    edited[src_t.long()] = True
    for i, r in enumerate(src):
        assert torch.equal(y[r].view(torch.int16), ys[i].view(torch.int16)), f"stream_edit: y of row {r}"
        assert torch.equal(mean[r:r + 1].view(torch.int32), ms[i:i + 1].view(torch.int32)) and \
            torch.equal(rstd[r:r + 1].view(torch.int32), rs[i:i + 1].view(torch.int32)), f"stream_edit: mean / rstd of row {r}"
    yb = y.view(torch.int16)
    for s0, s1 in slices(rows + 1, E):
        assert torch.equal((yb[s0:s1] != W.SENT16).any(1), edited[s0:s1]), f"stream_edit: y rows [{s0}, {s1}) outside the list"
    assert torch.equal(mean.view(torch.int32) != W.SENT32, edited) and torch.equal(rstd.view(torch.int32) != W.SENT32, edited)
    for u0, u1 in chunks:
        before = rand_units(74, u0, (u1 - u0, E), torch.float32, 2.0, 0.5)
        for i, r in enumerate(src):
            if u0 <= r < u1:
                before[r - u0] = after[i]
        assert torch.equal(xb[u0:u1], before.view(torch.int32)), f"stream_edit: rows [{u0}, {u1}) outside the list changed"
    # the token selector: every row whose token is in the set
    tok = torch.zeros(rows, dtype=torch.int64, device="cuda")
    tok[src_t.long()] = 5
    x_sel = after.cpu().numpy()
    ops.stream_edit(x[:rows], SE.AXPBY, 1.0, -2.0, tokens=tok, token_set=1 << 5, src=vec)
    guard_ok("stream_edit by tokens")
    after2 = torch.stack([x[r] for r in src])
    want = SE.axpby_rows(x_sel, vec.cpu().numpy()[None, :], 1.0, -2.0)
    assert np.array_equal(after2.cpu().numpy().view(np.int32), want.view(np.int32)), "stream_edit by tokens: the edited rows"
    for u0, u1 in chunks:
        before = rand_units(74, u0, (u1 - u0, E), torch.float32, 2.0, 0.5)
        for i, r in enumerate(src):
            if u0 <= r < u1:
                before[r - u0] = after2[i]
        assert torch.equal(xb[u0:u1], before.view(torch.int32)), f"stream_edit by tokens: rows [{u0}, {u1}) outside the set changed"
    print("row kernels: stream_edit edits the listed rows on both sides of the boundaries and nothing else")
    del x


def test_add_positions():
    """ops.add_positions in place on x fp32 [820, 1024, 1280] (2^32 bytes in sequence 819): one fp32 addition per element,
    bit-equal to tests/_frontend_ref.py add_positions_ref on every chunk of sequences; pads on both sides of the 256-row
    sweeps, a last sequence that is mostly padding."""
    import _frontend_ref as R

    case = W.CASES["add_positions"]
    gate(case)
    B, T, E = (case.shape[x] for x in "BTE")
    chunks = W.chunk_list(B, T * E * 4)
    assert W.B32 // (T * E * 4) == 819
    g = torch.Generator(device="cuda").manual_seed(121)
    tokens = torch.randint(4, 24, (B, T), device="cuda", generator=g)
    tokens[:, 0] = 0
    for c in (255, 256, 257, 511, 512):
        tokens[::5, c] = 1
    tokens[B - 1, 300:] = 1
    tokens[1::7, 900:] = 1
    pos_emb = 0.1 * torch.randn(T + 2, E, device="cuda", generator=g)
    pos_emb[1] = 0.0
    x = alloc_sentinel(B, (T, E), torch.float32)
    fill_random(x[:B], chunks, seed=122)
    ops.add_positions(tokens, pos_emb, x[:B], 1)
    xb = x.view(torch.int32)
    assert bool((xb[B:] == W.SENT32).all()), "add_positions: store behind the last sequence"
    for u0, u1 in chunks:
        want = R.add_positions_ref(rand_units(122, u0, (u1 - u0, T, E), torch.float32), tokens[u0:u1], pos_emb, 1)
        assert torch.equal(xb[u0:u1], want.view(torch.int32)), f"add_positions: sequences [{u0}, {u1}) differ from the reference"
    del x
