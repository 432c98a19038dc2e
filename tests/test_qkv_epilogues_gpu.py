"""gemm9's own q / k (RoPE) and V^T epilogues (csrc/gemm9.hip: epilogue9_t, epilogue9_vt), one op at a time through
esmk_op_qkv_rope2 / esmk_op_qkv_rope_ln, in every form the engine launches: full-height and half-height tiles, the
one-launch q / k / v form, plain and LayerNorm fold, fp16 and bf16.  The reference is gemm8's untouched epilogue
(gemm_epi.h, epilogue8m): q scaling + rotary + head split of esm/multihead_attention.py:256-284, rotary_embedding.py:11-20
and the transposed, key-permuted V of the attention kernel — bit for bit.

Shapes: one 32-row piece (1, 32); T % 32 != 0 with a sequence boundary inside a piece (3, 50): the per-element V^T path;
a clipped last row tile (3, 160); T % 64 != 0, Tp > T (2, 763); and a two-head E = 128 model at 64 x 1024 / 64 x 1022
rows, where 256 full-height tiles fill the chip once and the tile-height rule keeps full-height tiles (aligned and
per-element V^T path).  Every case asserts the plan (esmk_debug_gemm_plan), so none silently runs another kernel."""
import ctypes
import math

import pytest
import torch

from esm_amd import _native as N
from esm_amd import ops

pytestmark = pytest.mark.gpu

EPI_QKV_ALL = 8
# (B, T, E, H, the rule's tile height for the two launches: 1 = half-height)
CASES = [(1, 32, 1280, 20, 1), (3, 50, 1280, 20, 1), (3, 160, 1280, 20, 1), (2, 763, 1280, 20, 1),
         (64, 1024, 128, 2, 0), (64, 1022, 128, 2, 0)]
IDS = [f"{c[0]}x{c[1]}_E{c[2]}" for c in CASES]
DTYPES = [torch.float16, torch.bfloat16]


def knob(v):
    N.check(N.lib.esmk_debug_set(b"qkv_one_launch", ctypes.c_double(v)))


def impl(i):
    N.check(N.lib.esmk_debug_gemm_impl(i, 0))


@pytest.fixture(autouse=True)
def _restore_choice():
    yield
    knob(-1)
    impl(0)


def plan(M, n, K, epi, fold):
    out = (ctypes.c_int32 * 4)()
    N.check(N.lib.esmk_debug_gemm_plan(M, n, K, epi, 4 if fold else 0, out))
    return out[0], out[1]


def assert_plans(M, E, fold, half):
    """q / k, v and the one-launch form all run gemm9; the two launches at the expected tile height."""
    assert plan(M, 2 * E, E, N.EPI_QKV_ROPE, fold) == (9, half)
    assert plan(M, E, E, N.EPI_V_T, fold) == (9, half)
    assert plan(M, 3 * E, E, EPI_QKV_ALL, fold) == (9, 1)


def operands(B, T, E, dtype, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
    a = torch.randn(B * T, E, device="cuda", generator=g).to(dtype)
    w = (torch.randn(3 * E, E, device="cuda", generator=g) * (scale / math.sqrt(E))).to(dtype)
    bias = 0.1 * scale * torch.randn(3 * E, device="cuda", generator=g)
    return a, w, bias


def run_plain(qkv, a, w, bias, B, T):
    q, k, vt = qkv(a, w, bias, B, T, log2_domain=True)
    return q.clone(), k.clone(), vt.clone()


def run_fold(qkv, a, w, bias, bias2, rstd, B, T, dtype):
    H = qkv.H
    Tp = (T + 63) // 64 * 64
    q = torch.empty((B, H, T, 64), dtype=dtype, device="cuda")
    k = torch.empty_like(q)
    vt = torch.zeros((B, H, 64, Tp), dtype=dtype, device="cuda")
    N.check(N.lib.esmk_op_qkv_rope_ln(qkv.h, N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(bias2), N.ptr(rstd), N.ptr(q), N.ptr(k),
                                      N.ptr(vt), B, T, 1, N.cur_stream()))
    return q, k, vt


def valid_vt(vt, T):
    """The columns of vt that hold keys: positions permute_keys16(t), t < T (the rest of Tp is padding)."""
    return vt[..., ops.permute_keys16(T).to(vt.device)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,T,E,H,half", CASES, ids=IDS)
def test_plain_form_equals_gemm8_bit_for_bit(B, T, E, H, half, dtype):
    """gemm9 forced (full-height tiles), the rule's two launches and the one launch against gemm8."""
    a, w, bias = operands(B, T, E, dtype)
    qkv = ops.QkvHandle(E, H, operand_dtype=dtype)
    M = B * T
    impl(8)
    assert plan(M, 2 * E, E, N.EPI_QKV_ROPE, False)[0] == 8 and plan(M, E, E, N.EPI_V_T, False)[0] == 8
    ref = run_plain(qkv, a, w, bias, B, T)
    assert all(torch.isfinite(x.float()).all() for x in ref)
    forms = []
    impl(9)
    knob(0)
    assert plan(M, 2 * E, E, N.EPI_QKV_ROPE, False) == (9, 0) and plan(M, E, E, N.EPI_V_T, False) == (9, 0)
    forms.append(("gemm9 full height", run_plain(qkv, a, w, bias, B, T)))
    impl(0)
    assert_plans(M, E, False, half)
    forms.append(("two launches", run_plain(qkv, a, w, bias, B, T)))
    knob(1)
    forms.append(("one launch", run_plain(qkv, a, w, bias, B, T)))
    for form, got in forms:
        for name, x, y in zip("q k vt".split(), ref, got):
            if name == "vt":
                x, y = valid_vt(x, T), valid_vt(y, T)
            assert torch.equal(x, y), (form, name, int((x != y).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,T,E,H,half", CASES, ids=IDS)
def test_fold_form_is_gemm8_times_a_power_of_two_row_scale(B, T, E, H, half, dtype):
    """Zero bias, no bias2, ln_rstd[m] = 2^k(m), k cycling over -2 .. 2: every operation of the fold epilogues scales
    exactly, so q, k and V^T must be the plain gemm8 result on the same operands times 2^k(row), bit for bit — this pins
    the row -> rstd map and every permutation.  The operands are scaled (|k|, |v| ~ 1e3, |q| ~ 2e2) so that results stay
    inside fp16's normal range; the exactness argument does not hold for a result whose plain or scaled value is below
    2^-14 (fp16 subnormal: the two roundings differ), so such an element — a few per million, fp16 only — is held to
    2^-22 instead: half a subnormal spacing (2^-25) of the plain rounding times 2^2, plus the rounding of the result."""
    a, w, _ = operands(B, T, E, dtype, scale=1024.0)
    zero = torch.zeros(3 * E, device="cuda")
    qkv = ops.QkvHandle(E, H, operand_dtype=dtype)
    M = B * T
    impl(8)
    ref = run_plain(qkv, a, w, zero, B, T)
    impl(0)
    kk = (torch.arange(M, device="cuda") % 5) - 2
    rstd = torch.zeros((M + 255) // 256 * 256, device="cuda")
    rstd[:M] = torch.exp2(kk.float())
    s = rstd[:M].view(B, 1, T, 1)
    want = [ref[0].float() * s, ref[1].float() * s, valid_vt(ref[2], T).float() * s.view(B, 1, 1, T)]
    assert_plans(M, E, True, half)
    lim = 65504.0 if dtype == torch.float16 else 3e38
    tiny = 2.0 ** -14 if dtype == torch.float16 else 0.0
    for mode, form in ((0, "two launches"), (1, "one launch")):
        knob(mode)
        got = run_fold(qkv, a, w, zero, None, rstd, B, T, dtype)
        got = [got[0], got[1], valid_vt(got[2], T)]
        for name, x, y, r in zip("q k vt".split(), want, got, (ref[0], ref[1], valid_vt(ref[2], T))):
            assert x.abs().max().item() <= lim, (form, name)
            normal = (r.float().abs() >= tiny) & (x.abs() >= tiny) | (r.float() == 0)
            assert (~normal).float().mean().item() < 1e-4, (form, name)
            assert torch.equal(x.to(dtype)[normal], y[normal]), (form, name, int((x.to(dtype) != y)[normal].sum()))
            if (~normal).any():
                assert (x - y.float())[~normal].abs().max().item() <= 2.0 ** -22, (form, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B,T,E,H,half", CASES, ids=IDS)
def test_fold_form_with_bias_and_bias2_same_bits_in_every_launch_form(B, T, E, H, half, dtype):
    """Real rstd, bias and bias2: the two launches (half-height or full-height tiles by the rule) and the one launch
    (half-height) agree bit for bit; the values are the fold's, within the rounding of the operand dtype, against fp64."""
    a, w, bias = operands(B, T, E, dtype)
    g = torch.Generator(device="cuda").manual_seed(7)
    bias2 = 0.1 * torch.randn(3 * E, device="cuda", generator=g)
    M = B * T
    rstd = torch.zeros((M + 255) // 256 * 256, device="cuda")
    rstd[:M] = 0.5 + torch.rand(M, device="cuda", generator=g)
    qkv = ops.QkvHandle(E, H, operand_dtype=dtype)
    assert_plans(M, E, True, half)
    outs = []
    for mode in (0, 1):
        knob(mode)
        q, k, vt = run_fold(qkv, a, w, bias, bias2, rstd, B, T, dtype)
        outs.append((q, k, valid_vt(vt, T)))
    for name, x, y in zip("q k vt".split(), outs[0], outs[1]):
        assert torch.isfinite(x.float()).all(), name
        assert torch.equal(x, y), (name, int((x != y).sum()))
    # V against fp64 on a slice of the rows: one rounding to the operand dtype (half an ulp: 2^-11 / 2^-8 of the value)
    # on top of the fp32 accumulation, bounded in any summation order by (K + 2) 2^-24 sum |a_k w_k| rstd
    rows = torch.arange(0, M, max(1, M // 64), device="cuda")
    r64, b64 = rstd[rows].double()[:, None], (bias[2 * E:] + bias2[2 * E:]).double()
    v64 = (a[rows].double() @ w[2 * E:].double().t()) * r64 + b64
    mag = (a[rows].double().abs() @ w[2 * E:].double().abs().t()) * r64 + b64.abs()
    got = outs[0][2].permute(0, 3, 1, 2).reshape(M, E)[rows].double()  # [B,H,64,T] -> [M, E]
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    excess = (got - v64).abs() - (eps * v64.abs() + (E + 2) * 2.0 ** -24 * mag * (1 + eps))
    assert (excess <= 0).all(), float(excess.max())


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "ln_fold"])
def test_row_positions_packed_equals_each_sequence_alone(fold, monkeypatch):
    """The row_pos path of the RoPE epilogue (token-packed batches): a mixed-length batch through forward_varlen gives
    every sequence the bits it gets alone."""
    import esm
    from esm_amd.synth import skip_param_init, synth_esm2_state_dict

    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1" if fold else "0")
    L, E, H = 2, 1280, 20
    sd = synth_esm2_state_dict(L, E, H, seed=11)
    with skip_param_init():
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(sd)
    model = model.cuda()
    lens = [150, 33, 97, 128, 64, 2]
    gen = torch.Generator().manual_seed(3)
    toks = torch.full((len(lens), max(lens)), 1, dtype=torch.int64)  # <pad>
    for b, n in enumerate(lens):  # <cls> residues <eos> <pad>...
        toks[b, 0], toks[b, n - 1] = 0, 2
        if n > 2:
            toks[b, 1:n - 1] = torch.randint(4, 24, (n - 2,), generator=gen)
    with torch.no_grad():
        pk = model.forward_varlen(toks, repr_layers=[1, L], min_saving=None)
        for b, n in enumerate(lens):
            one = model(toks[b:b + 1, :n].cuda(), repr_layers=[1, L])
            for layer in (1, L):
                assert torch.equal(pk["representations"][layer][b, :n], one["representations"][layer][0]), (b, n, layer)
            assert torch.equal(pk["logits"][b, :n], one["logits"][0]), (b, n)
