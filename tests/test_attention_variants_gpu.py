"""Every form of the attention core the engine launches, one kernel at a time, against a plain fp64 softmax.

The engine runs six forms of the flash-attention kernels (csrc/attention.hip, csrc/attention128.hip): head_dim 64 and
128 on padded batches with the per-sequence `seq_info` (all-pad tail key tiles skipped, padded query rows in the place
of the last real row), the f16x3 context layout (hi | hi | lo), the MSA column fill mode (scores of flagged keys
REPLACED by -10000) and the probability kernels of need_head_weights / contacts / col_attentions.  Whole-model tests
see these only through the fp16 GEMM floor, and bit-equality between layouts cannot catch an error all layouts
share; here each form is reached through esmk_op_attention_ex / esmk_op_attention_probs_ex and compared with

    s = q k^T (+ key_bias | masked_fill(flag, -10000));  p = softmax(s);  o = p v;  lse = logsumexp(s)

in fp64 on the kernel's own operand values: q_effective from ops.to_log2_domain, k and v rounded to the operand dtype.
The tiles are 64 keys and 128 query rows (4 waves of 32): the lengths sit on and next to those edges, and B*H is chosen
so that the XCD-grouped grid (bh in groups of 8) runs its remainder branch alone, its main branch alone and both."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
NEG = float("-inf")


def _eps(dt):
    return 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def _inputs(ops, B, H, T, D, dt, scale, seed):
    """q (log2-domain operand + its natural-domain value), k, v; raw scores ~ N(0, (4.8 scale)^2): scale 4 reaches
    +-100 and makes the online softmax move its offset by large steps."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    kscale = 0.6 * math.sqrt(64.0 / D)
    qk, q = ops.to_log2_domain(torch.randn(B, H, T, D, device="cuda", generator=g) * scale, dt)
    k = (torch.randn(B, H, T, D, device="cuda", generator=g) * kscale).to(dt)
    v = torch.randn(B, H, T, D, device="cuda", generator=g).to(dt)
    return qk, q, k, v


def _ref(q, k, v, key_bias=None, fill=None):
    """fp64 reference: multihead_attention.py:357 (bmm q k^T; q already carries the head scaling), :368-374 (key
    padding: masked_fill(-inf), here the equivalent additive 0 / -inf bias), :379 (softmax), :387 (bmm with v), or for
    the MSA column form axial_attention.py:209-215 (masked_fill(padding_mask, -10000), only when the batch has a pad:
    msa_transformer.py:152-154) and :217-219.  Returns probabilities [B,H,T,T], ctx [B,H,T,D] and the natural lse."""
    s = q.double() @ k.double().transpose(-1, -2)
    if key_bias is not None:
        s = s + key_bias.double()[:, None, None, :]
    if fill is not None:
        s = s.masked_fill(fill.bool()[:, None, None, :], -10000.0)
    p = torch.softmax(s, dim=-1)
    return p, p @ v.double(), torch.logsumexp(s, dim=-1)


def _merge(o):
    """[B,H,T,D] -> the kernels' ctx layout [B*T, H*D] (multihead_attention.py:394)."""
    B, H, T, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * T, H * D)


def _seq_info(key_bias):
    """(#pads, 1 + index of the last non-pad token) per sequence, as seq_stats_kernel writes it."""
    pad = torch.isinf(key_bias)
    T = key_bias.shape[1]
    idx = torch.arange(1, T + 1, device=key_bias.device)
    last = torch.where(pad, torch.zeros_like(idx), idx).max(dim=1).values
    return torch.stack([pad.sum(1), last], dim=1).to(torch.int32).contiguous()


def _check_ctx(ctx, o_ref, dt, rows=None):
    ref = _merge(o_ref)
    got = ctx.double()
    if rows is not None:
        ref, got = ref[rows], got[rows]
    err = (got - ref).abs().max().item()
    assert err <= 4 * _eps(dt) * max(1.0, ref.abs().max().item()), err


def _check_lse(lse, lse_ref, mask=None):
    if mask is not None:
        lse, lse_ref = lse[mask], lse_ref[mask]
    err = (lse.double() - lse_ref).abs().max().item()
    assert err <= 1e-3 * max(1.0, lse_ref.abs().max().item()), err


def _check_probs(probs, p_ref, out_dtype):
    """Within 2e-3 max p + 1e-6 of the fp64 map; a map stored in fp16 / bf16 may also carry its own rounding."""
    assert torch.isfinite(probs).all()
    got = probs.double()
    tol = 2e-3 * p_ref.max().item() + 1e-6
    if out_dtype != torch.float32:
        tol = tol + _eps(out_dtype) * p_ref.abs()
    assert ((got - p_ref).abs() <= tol).all(), (got - p_ref).abs().max().item()


# ---- plain sequences: every length edge, every grid branch, both head dims and dtypes ------------------------------

_TS = [1, 2, 33, 63, 64, 65, 127, 128, 129, 257, 1024]
_BH = [(1, 1), (1, 7), (2, 4), (3, 3), (1, 41), (2, 20), (1, 40)]   # B*H = 1, 7, 8, 9, 41, 40, 40
_CASES = []
for _j, (_D, _dt) in enumerate([(64, torch.float16), (64, torch.bfloat16), (128, torch.float16), (128, torch.bfloat16)]):
    for _i, _T in enumerate(_TS):
        _B, _H = _BH[(_i + 2 * _j) % len(_BH)]
        _CASES.append((_B, _H, _T, _D, _dt, (0.6, 4.0)[(_i + _j) % 2]))
_CASES += [(1, 2, 4100, 64, torch.float16, 4.0), (1, 1, 4100, 128, torch.bfloat16, 0.6)]


@pytest.mark.parametrize("B,H,T,D,dt,scale", _CASES)
def test_forward_and_probs_against_fp64(ops, B, H, T, D, dt, scale):
    qk, q, k, v = _inputs(ops, B, H, T, D, dt, scale, seed=T * 7 + B * H + D)
    ctx, lse = ops.attention(qk, k, ops.make_vt(v), want_lse=True)
    assert ctx.shape == (B * T, H * D)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    p_ref, o_ref, lse_ref = _ref(q, k, v)
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)
    out_dtype = torch.float32 if (T + D) % 2 else dt
    probs = ops.attention_probs(qk, k, lse, out_dtype=out_dtype)
    _check_probs(probs[:, 0], p_ref, out_dtype)


@pytest.mark.parametrize("dt", DT)
def test_head_dim_128_rescale_spike(ops, dt):
    """test_attention_rescale_spike for head_dim 128: keys that dominate one query late in the sweep force large
    moves of the running maximum (and the rescale of all four 32x32 accumulators)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    B, H, T, D = 1, 3, 512, 128
    q = torch.randn(B, H, T, D, device="cuda", generator=g) * 0.2
    k = torch.randn(B, H, T, D, device="cuda", generator=g) * 0.2
    k[0, :, 400] = q[0, :, 17] * 40.0
    k[0, :, 130] = q[0, :, 300] * 25.0
    k[0, :, 500] = q[0, :, 3] * 60.0
    (qk, q), k = ops.to_log2_domain(q, dt), k.to(dt)
    v = torch.randn(B, H, T, D, device="cuda", generator=g).to(dt)
    ctx, lse = ops.attention(qk, k, ops.make_vt(v), want_lse=True)
    p_ref, o_ref, lse_ref = _ref(q, k, v)
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)
    _check_probs(ops.attention_probs(qk, k, lse)[:, 0], p_ref, torch.float32)


# ---- padded batches with seq_info --------------------------------------------------------------------------------

def _padded_batch(T):
    """One sequence per padding pattern: none; trailing with kv_end 64, 65, 127, 128 (tile-aligned and not);
    interior pads including a run over one whole 64-key tile; padding only.  Returns key_bias [B,T] and, per
    sequence, its length when the pads are all trailing (None otherwise)."""
    kv = [T, 64, 65, 127, 128]
    B = len(kv) + 2
    bias = torch.zeros(B, T, device="cuda")
    for b, e in enumerate(kv):
        bias[b, e:] = NEG
    bias[5, 3] = bias[5, 17] = NEG
    bias[5, 64:128] = NEG
    bias[5, T - 5:] = NEG
    bias[6, :] = NEG
    return bias, kv + [None, None]


@pytest.mark.parametrize("D,dt,T,H,scale", [
    (64, torch.float16, 257, 1, 0.6), (64, torch.bfloat16, 200, 3, 4.0), (64, torch.float16, 1024, 2, 4.0),
    (128, torch.float16, 257, 1, 4.0), (128, torch.bfloat16, 200, 3, 0.6), (128, torch.bfloat16, 1024, 2, 4.0),
])
def test_padded_batch_with_seq_info(ops, D, dt, T, H, scale):
    """The padded-batch form esmk_forward launches: real rows against the fp64 reference and bit-identical to the
    sequence run alone (T = its length, no bias: the kernel comment's claim); every output finite, padded query rows
    included; a sequence of padding only gives ctx 0 (and lse 0 — for head_dim 64 every padding-only wave does);
    the maps have exact zeros on padded rows and columns, and the padding-only map is all zeros, never NaN."""
    bias, lens = _padded_batch(T)
    B = bias.shape[0]
    qk, q, k, v = _inputs(ops, B, H, T, D, dt, scale, seed=T + D + H)
    seq_info = _seq_info(bias)
    assert seq_info[6].tolist() == [T, 0] and seq_info[0].tolist() == [0, T]
    ctx, lse = ops.attention(qk, k, ops.make_vt(v), bias, want_lse=True, seq_info=seq_info)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    p_ref, o_ref, lse_ref = _ref(q, k, v, bias)
    real = ~torch.isinf(bias)                                      # [B,T] query rows of real tokens
    _check_ctx(ctx, o_ref, dt, rows=real.reshape(-1))
    _check_lse(lse, lse_ref, mask=real[:, None, :].expand(B, H, T))
    ctx3 = ctx.view(B, T, H * D)
    assert (ctx3[6] == 0).all() and (lse[6] == 0).all()
    if D == 64:  # waves (32 query rows) at or past max(kv_end, 1) do no work and write zeros
        for b in range(B):
            q_end = max(int(seq_info[b, 1]), 1)
            first = (q_end + 31) // 32 * 32
            assert (ctx3[b, first:] == 0).all() and (lse[b, :, first:] == 0).all(), b
    for b, L in enumerate(lens):
        if L is None:
            continue
        alone = ops.attention(qk[b:b + 1, :, :L].contiguous(), k[b:b + 1, :, :L].contiguous(),
                              ops.make_vt(v[b:b + 1, :, :L].contiguous()), want_lse=True)
        assert torch.equal(ctx3[b, :L], alone[0]), (b, L)
        assert torch.equal(lse[b, :, :L], alone[1][0]), (b, L)
    keep = real.double()
    p_ref = torch.nan_to_num(p_ref) * keep[:, None, :, None] * keep[:, None, None, :]
    for out_dtype in (torch.float32, dt):
        probs = ops.attention_probs(qk, k, lse, bias, out_dtype=out_dtype)[:, 0]
        _check_probs(probs, p_ref, out_dtype)
        assert (probs[p_ref == 0] == 0).all()                       # padded rows and columns: exact zeros
        assert (probs[6] == 0).all()


# ---- MSA column attention (fill mode) ------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("Bm,C,H,R,scale", [(1, 3, 2, 33, 0.6), (2, 2, 3, 129, 4.0), (1, 4, 2, 64, 0.6),
                                           (1, 1, 4, 257, 4.0), (2, 3, 1, 1, 0.6), (1, 2, 2, 65, 0.6)])
def test_msa_column_fill(ops, dt, Bm, C, H, R, scale):
    """Column attention over the R rows of each (batch, column) "sequence" (axial_attention.py:185-219).
    - flags with any_pad = 0 (msa_transformer.py:152-154 drops the mask): the same bits as no mask;
    - any_pad = 1: the flagged scores are REPLACED by -10000, not added to;
    - a column whose keys are all flagged: a uniform softmax, the plain average of v (-inf would give NaN);
    - queries whose real scores all lie below -10000: the weight sits on the flagged keys;
    and the maps land in col_attentions [Bm, L, H, C, R, R] with query rows NOT zeroed."""
    B, D = Bm * C, 64
    qk, q, k, v = _inputs(ops, B, H, R, D, dt, scale, seed=R + B + H)
    flags = torch.zeros(B, R, device="cuda")
    if R > 1:
        flags[0, R // 2] = flags[0, R - 1] = 1.0
    flags[B - 1, :] = 1.0                                            # every key of one column flagged
    if B > 2:
        flags[1, :: 3] = 1.0
    if R >= 8:  # sequence 0: query rows 0..3 score below -10000 against every key that is not flagged
        n = torch.ones(D, device="cuda")
        n[1::2] = -1
        kk = k.float()
        kk[0, :, :] = n * 1.0 + 0.1 * torch.randn(H, R, D, device="cuda")
        k = kk.to(dt)
        q = q.clone()
        q[0, :, :4] = n * -200.0                                     # raw scores about -12800
        qk, q = ops.to_log2_domain(q, dt)
    vt = ops.make_vt(v)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    plain = ops.attention(qk, k, vt, want_lse=True)
    off = ops.attention(qk, k, vt, flags, want_lse=True, fill_any_pad=zero)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    ctx, lse = ops.attention(qk, k, vt, flags, want_lse=True, fill_any_pad=one)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    p_ref, o_ref, lse_ref = _ref(q, k, v, fill=flags)
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)
    mean_v = _merge(v.double().mean(dim=2, keepdim=True).expand(B, H, R, D)).view(B, R, H * D)[B - 1]
    assert (ctx.view(B, R, H * D)[B - 1].double() - mean_v).abs().max().item() <= 4 * _eps(dt) * max(
        1.0, mean_v.abs().max().item())
    if R >= 8:
        fk = flags[0].bool()
        assert (p_ref[0, :, :4][..., fk].sum(-1) > 1 - 1e-9).all()   # the reference's weight: all on flagged keys
        want = v[0, :, fk].double().mean(dim=1)                      # [H, D]
        got = ctx.view(B, R, H, D)[0, :4].double()
        assert (got - want[None]).abs().max().item() <= 4 * _eps(dt) * max(1.0, want.abs().max().item())
    L = 2
    probs = ops.attention_probs(qk, k, lse, flags, layer=1, num_layers=L, fill_any_pad=one, msa_C=C)
    assert probs.shape == (Bm, L, H, C, R, R)
    got = probs[:, 1].permute(0, 2, 1, 3, 4).reshape(B, H, R, R)
    _check_probs(got, p_ref, torch.float32)
    assert (got[B - 1] - 1.0 / R).abs().max().item() <= 2e-3 / R + 1e-6   # uniform rows, none zeroed


# ---- f16x3 context layout ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,T,padded", [(1, 1, 65, False), (2, 4, 129, False), (1, 9, 257, False),
                                          (7, 1, 257, True), (7, 3, 200, True)])
def test_f16x3_context(ops, B, H, T, padded):
    """hi | hi | lo per head: the two hi blocks are the same bits, lo is the rounding remainder (at most half an ulp of
    hi) and hi + lo is no farther from the fp64 reference than hi alone.  The K loop is shared with the plain kernel
    and the lse is bit-equal; hi itself is within ONE ulp of the plain kernel's ctx, not bit-equal: the normalised
    value o * inv reaches fp16 either as one v_fma_mixlo_f16 (the exact product rounded once) or as v_mul_f32 then
    v_cvt_pk_f16_f32 (rounded to fp32 first), and the compiler picks per element, differently in the two
    instantiations (X3 keeps the fp32 product for lo).  The two roundings differ only on fp16 ties."""
    D, dt = 64, torch.float16
    bias, seq_info = None, None
    if padded:
        bias, _ = _padded_batch(T)
        seq_info = _seq_info(bias)
    qk, q, k, v = _inputs(ops, B, H, T, D, dt, 0.6 if B % 2 else 4.0, seed=3 * T + H)
    vt = ops.make_vt(v)
    ctx3, lse3 = ops.attention(qk, k, vt, bias, want_lse=True, seq_info=seq_info, x3=True)
    ctx, lse = ops.attention(qk, k, vt, bias, want_lse=True, seq_info=seq_info)
    parts = ctx3.view(B * T, H, 3, D)
    hi, hi2, lo = parts[:, :, 0], parts[:, :, 1], parts[:, :, 2]
    assert torch.equal(hi, hi2)
    assert torch.equal(lse3, lse)
    h = hi.float()
    _, e = torch.frexp(h)
    ulp = torch.where(h == 0, torch.full_like(h, 2.0 ** -24), torch.exp2((e - 11).float()).clamp_min(2.0 ** -24))
    plain = ctx.view(B * T, H, D).float()
    assert ((h - plain).abs() <= ulp).all()
    assert (h != plain).float().mean().item() < 1e-3                 # ties only
    assert (lo.float().abs() <= ulp / 2).all()
    _, o_ref, _ = _ref(q, k, v, bias)
    rows = slice(None) if bias is None else (~torch.isinf(bias)).reshape(-1)
    ref = _merge(o_ref).view(B * T, H, D)[rows]
    e_hi = (hi[rows].double() - ref).norm().item()
    e_sum = (hi[rows].double() + lo[rows].double() - ref).norm().item()
    assert e_sum <= e_hi, (e_sum, e_hi)
