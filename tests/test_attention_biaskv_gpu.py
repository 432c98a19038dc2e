"""The attention kernel with a learned null key / value pair (ESM-1's add_bias_kv; csrc/attention.hip, NK) alone, through
esmk_op_attention_biaskv, against a plain fp64 softmax over T + 1 keys:

    s = [q k^T (+ key_bias) | q bias_k];  p = softmax(s);  o = p [v ; bias_v];  lse = logsumexp(s)

on the kernel's own operand values, in the style and with the mode-0 bounds of tests/test_attention_variants_gpu.py
(`_check_ctx`, `_check_lse`, `_check_probs` there).  The map kernel is untouched by the feature: it computes
exp(s - lse) over the T real keys, and because lse includes the null key that IS the reference's map with the null column
dropped — checked here, which is also why lse is compared on every case."""
import math

import pytest
import torch

from test_attention_variants_gpu import _check_ctx, _check_lse, _check_probs, _inputs, _merge, _seq_info

pytestmark = pytest.mark.gpu
NEG = float("-inf")


@pytest.fixture(scope="module")
def ops():
    from esm_amd import ops as _ops

    return _ops


def _null(H, dt, seed, q=None):
    """bias_k at the scale of the key rows, bias_v at the scale of the value rows.  q given: each head's bias_k also gets the
    component along that head's first query row that adds 8 to that row's null-key score, so the null key holds real mass in
    at least one row of every case, the one-row cases included."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bk = torch.randn(H, 64, device="cuda", generator=g) * 0.6
    if q is not None:
        q0 = q[0, :, 0, :].float()
        bk = bk + 8.0 * q0 / (q0 * q0).sum(-1, keepdim=True)
    bv = torch.randn(H, 64, device="cuda", generator=g).to(dt)
    return bk.to(dt), bv


def _ref(q, k, v, bk, bv, key_bias=None):
    """fp64: probabilities over the T real keys [B,H,T,T], the null key's probability [B,H,T], ctx, natural lse."""
    s = q.double() @ k.double().transpose(-1, -2)
    if key_bias is not None:
        s = s + key_bias.double()[:, None, None, :]
    s0 = (q.double() * bk.double()[None, :, None, :]).sum(-1, keepdim=True)
    p = torch.softmax(torch.cat([s, s0], dim=-1), dim=-1)
    o = p[..., :-1] @ v.double() + p[..., -1:] * bv.double()[None, :, None, :]
    return p[..., :-1], p[..., -1], o, torch.logsumexp(torch.cat([s, s0], dim=-1), dim=-1)


_TS = [1, 63, 64, 65, 127, 128, 129, 300]
_BH = [(1, 1), (1, 7), (2, 4), (3, 3), (1, 9), (2, 20)]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T", _TS)
def test_null_key_forward_and_maps_against_fp64(ops, T, dt):
    B, H = _BH[(_TS.index(T) + (dt == torch.bfloat16)) % len(_BH)]
    scale = (0.6, 4.0)[_TS.index(T) % 2]
    qk, q, k, v = _inputs(ops, B, H, T, 64, dt, scale, seed=T * 11 + B * H)
    bk, bv = _null(H, dt, seed=T, q=q)
    ctx, lse = ops.attention_biaskv(qk, k, ops.make_vt(v), bk, bv)
    assert ctx.shape == (B * T, H * 64)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    p_ref, p0_ref, o_ref, lse_ref = _ref(q, k, v, bk, bv)
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)
    # the unchanged map kernel on the null-key lse: the reference's "null column dropped" map, rows summing to 1 - p0
    probs = ops.attention_probs(qk, k, lse)[:, 0]
    _check_probs(probs, p_ref, torch.float32)
    assert ((1 - probs.double().sum(-1)) - p0_ref).abs().max().item() <= 2e-3 * (T + 1)
    assert p0_ref.max().item() > 0.05  # the case has rows in which the null key matters


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T", _TS)
def test_null_key_padded_batch_with_seq_info(ops, T, dt):
    """Padded-batch form (key_bias + seq_info, what esmk_forward launches): trailing pads at every kv_end that fits, one
    sequence with interior pads, one of padding only.  Real rows against fp64; everything finite; the null key is never
    masked."""
    ends = sorted({e for e in (T, 1, 63, 64, 65, 127, 128) if e <= T})
    B, H = len(ends) + 2, 2
    bias = torch.zeros(B, T, device="cuda")
    for b, e in enumerate(ends):
        bias[b, e:] = NEG
    if T > 4:
        bias[B - 2, 1] = bias[B - 2, T - 2] = NEG
        bias[B - 2, T // 2:T // 2 + 70] = NEG
    bias[B - 1, :] = NEG
    qk, q, k, v = _inputs(ops, B, H, T, 64, dt, 0.6 if T % 2 else 4.0, seed=T + 5)
    bk, bv = _null(H, dt, seed=T + 1, q=q)
    ctx, lse = ops.attention_biaskv(qk, k, ops.make_vt(v), bk, bv, key_bias=bias, seq_info=_seq_info(bias))
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()          # padded rows and the all-padding sequence too
    p_ref, p0_ref, o_ref, lse_ref = _ref(q, k, v, bk, bv, bias)
    real = ~torch.isinf(bias)
    _check_ctx(ctx, o_ref, dt, rows=real.reshape(-1))
    _check_lse(lse, lse_ref, mask=real[:, None, :].expand(B, H, T))
    probs = ops.attention_probs(qk, k, lse, key_bias=bias)[:, 0]
    keep = (real[:, None, :, None] & real[:, None, None, :]).double()
    _check_probs(probs, p_ref * keep, torch.float32)
    assert (probs[B - 1] == 0).all()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_null_key_without_seq_info_masks_keys_only(ops, dt):
    """key_bias alone (no seq_info): every key tile runs, pads are masked, the null key is not."""
    B, H, T = 2, 3, 200
    bias = torch.zeros(B, T, device="cuda")
    bias[0, 150:] = NEG
    bias[1, 7] = NEG
    qk, q, k, v = _inputs(ops, B, H, T, 64, dt, 4.0, seed=77)
    bk, bv = _null(H, dt, seed=78)
    ctx, lse = ops.attention_biaskv(qk, k, ops.make_vt(v), bk, bv, key_bias=bias)
    _, _, o_ref, lse_ref = _ref(q, k, v, bk, bv, bias)
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T", [65, 300])
def test_dominant_null_key(ops, T, dt):
    """A null key whose probability is at least 2^20 times that of every real key: ctx ~ bias_v, lse finite (the fold
    rescales against the offset instead of overflowing)."""
    B, H = 2, 2
    g = torch.Generator(device="cuda").manual_seed(T)
    qk, q = ops.to_log2_domain(torch.randn(B, H, T, 64, device="cuda", generator=g) * 0.05 + 1.0, dt)
    k = (torch.randn(B, H, T, 64, device="cuda", generator=g) * 0.05).to(dt)
    v = torch.randn(B, H, T, 64, device="cuda", generator=g).to(dt)
    bk = torch.full((H, 64), 1.0, device="cuda").to(dt)    # q . bias_k ~ 64, q . k ~ 0 +- 0.5
    bv = torch.randn(H, 64, device="cuda", generator=g).to(dt)
    p_ref, p0_ref, o_ref, lse_ref = _ref(q, k, v, bk, bv)
    assert (p0_ref.log() - p_ref.max(-1).values.log()).min().item() >= 20 * math.log(2.0)
    ctx, lse = ops.attention_biaskv(qk, k, ops.make_vt(v), bk, bv)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    _check_ctx(ctx, o_ref, dt)
    _check_lse(lse, lse_ref)
    want = bv.double()[None, :, None, :].expand(B, H, T, 64)
    assert (ctx.double() - _merge(want)).abs().max().item() <= 4 * (2.0 ** -11 if dt == torch.float16 else 2.0 ** -8) * max(1.0, want.abs().max().item())


def test_entry_validation(ops):
    from esm_amd import _native as N

    z = torch.zeros(64, device="cuda", dtype=torch.float16)
    rc = N.lib.esmk_op_attention_biaskv(N.ptr(z), N.ptr(z), N.ptr(z), None, None, None, N.ptr(z), N.ptr(z), None, 1, 1, 1, 64,
                                        N.F16, None)
    assert rc != 0 and "null argument" in N.lib.esmk_last_error().decode()
    rc = N.lib.esmk_op_attention_biaskv(N.ptr(z), N.ptr(z), N.ptr(z), None, None, N.ptr(z), N.ptr(z), N.ptr(z), None, 1, 1, 70,
                                        64, N.F16, None)
    assert rc != 0 and "Tp" in N.lib.esmk_last_error().decode()
