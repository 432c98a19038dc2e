"""The fp64 reference of tests/_gemm_ref.py, pinned without a GPU:
  * composed as the engine composes its launches (q / k / v with keep, tied scores in S slices, softmax, context,
    out-proj through the row map), it reproduces oracle.msa_oracle.row_attention / column_attention in fp64;
  * the head_dim-128 q / k reference, read through the packed weight image and the QKV epilogue's slice arithmetic
    (gemm_epi.h), reproduces the natural-order rotary embedding on un-permuted weights;
  * each wrong variant of a layout or a contraction moves the output by at least 10x the per-element bound, so the
    GPU tests that use that bound would see it."""
import math

import pytest
import torch

from oracle import msa_oracle
import _gemm_ref as G

D, HEADS = 128, 2


def make_sd(seed=0, p="a."):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        sd[p + n + ".weight"] = torch.randn(D, D, generator=g, dtype=torch.float64) / math.sqrt(D)
        sd[p + n + ".bias"] = 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    return sd


def make_x(R, C, B, seed=1):
    return torch.randn(R, C, B, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def make_pad(R, C, B, seed=2):
    g = torch.Generator().manual_seed(seed)
    pad = torch.zeros(B, R, C, dtype=torch.bool)
    for b in range(B):  # a padded tail in some rows, and a column padded in row 0 only
        pad[b, :, C - 1 - b:] = True
        pad[b, 0, torch.randint(0, C, (1,), generator=g)] = True
    return pad


def W(sd, n, p="a."):
    return sd[p + n + ".weight"], sd[p + n + ".bias"]


def composed_row(sd, x, pad, S):
    R, C, B, _ = x.shape
    keep = None if pad is None else (~pad).double()
    q, _ = G.msa_proj(x, *W(sd, "q_proj"), HEADS, keep=keep, sc=(64 ** -0.5) / math.sqrt(R))
    k, _ = G.msa_proj(x, *W(sd, "k_proj"), HEADS)
    v, _ = G.msa_proj(x, *W(sd, "v_proj"), HEADS)
    parts, _ = G.row_scores(q, k, S)
    probs, _ = G.row_softmax(parts, None if pad is None else pad[:, 0])
    ctx, _ = G.row_context(probs, v)
    out, _ = G.dense(G.rows_of(ctx.reshape(R, C, B, D)), *W(sd, "out_proj"))
    return G.from_rows(out, R, C, B), probs


def composed_column(sd, x):
    R, C, B, _ = x.shape
    xr = G.col_rows_of(x)

    def proj(n, sc=1.0):
        y, _ = G.dense(xr, *W(sd, n))
        return (y * sc).view(B, C, R, HEADS, 64).permute(2, 1, 0, 3, 4)

    ctx = G.column_attention_core(proj("q_proj", 64 ** -0.5), proj("k_proj"), proj("v_proj"))
    y, by = G.dense(ctx.permute(2, 1, 0, 3, 4).reshape(B * C * R, D), *W(sd, "out_proj"))
    out, _ = G.resid_rowmap(torch.zeros(B * R * C, D, dtype=torch.float64), y, by, B, R, C)
    return G.from_rows(out, R, C, B)


@pytest.mark.parametrize("R,C,B,S,padded", [(1, 5, 1, 1, False), (1, 7, 2, 1, True), (4, 9, 1, 1, True),
                                           (4, 9, 2, 2, False), (6, 5, 2, 3, True), (8, 3, 1, 8, True)])
def test_composed_row_attention_is_the_oracle(R, C, B, S, padded):
    sd, x = make_sd(), make_x(R, C, B)
    pad = make_pad(R, C, B) if padded else None
    want, want_probs = msa_oracle.row_attention(sd, "a.", x, HEADS, pad)
    got, probs = composed_row(sd, x, pad, S)
    # the only difference: the q scale d^-1/2 / sqrt(R) as the fp32 number the kernel multiplies by
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    assert (probs - want_probs).abs().max().item() <= 1e-6


@pytest.mark.parametrize("R,C,B", [(1, 5, 2), (3, 4, 1), (5, 7, 2)])
def test_composed_column_attention_is_the_oracle(R, C, B):
    sd, x = make_sd(3), make_x(R, C, B, seed=4)
    want, _ = msa_oracle.column_attention(sd, "a.", x, HEADS, None)
    got = composed_column(sd, x)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def natural_rope(y, inv_freq, pos):
    """tests/test_kernels_gpu.py _rope_ref (rotary_embedding.py:11-20,47-61) at positions `pos`, y [T, H, d]."""
    freqs = torch.einsum("i,j->ij", pos.double(), inv_freq.double())
    emb = torch.cat((freqs, freqs), dim=-1)[:, None, :]
    y1, y2 = y.chunk(2, dim=-1)
    return y * emb.cos() + torch.cat((-y2, y1), dim=-1) * emb.sin()


def kernel_slices_128(x, w_img, b_img, cos, sin, pos, H):
    """The QKV epilogue of a 128-wide head as gemm_epi.h states it, on the packed weight image: slice sl = columns
    [64 sl, 64 sl + 64) of the head, column c < 32 pairs with c + 32, cos / sin index 32 sl + c; stored in place."""
    y = (x @ w_img.T + b_img).view(-1, H, 2, 64)
    c, s = cos.double()[pos].view(-1, 1, 2, 32), sin.double()[pos].view(-1, 1, 2, 32)
    a1, a2 = y[..., :32], y[..., 32:]
    return torch.cat((a1 * c - a2 * s, a2 * c + a1 * s), -1).view(-1, H, 128)


def test_head_dim_128_reference_is_the_natural_rotary():
    g = torch.Generator().manual_seed(5)
    T, H, K = 37, 3, 64
    x = torch.randn(T, K, generator=g, dtype=torch.float64)
    w = torch.randn(H * 128, K, generator=g, dtype=torch.float64)
    b = torch.randn(H * 128, generator=g, dtype=torch.float64)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    pos = torch.randperm(T, generator=g)
    cos, sin = G.rope_tables(inv_freq, T)
    want = natural_rope((x @ w.T + b).view(T, H, 128), inv_freq, pos)
    y, by = G.dense(x, w, b)
    got, _ = G.rope(y.view(T, H, 128), by.view(T, H, 128), cos, sin, pos)
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()  # fp32 tables against fp64 angles
    # the reference's layout = what the epilogue computes on the packed weight image
    img = kernel_slices_128(x, G.weight_image(w, H), G.weight_image(b[:, None], H)[:, 0], cos, sin, pos, H)
    lay = G.qk_layout(got[None])[0].permute(1, 0, 2)  # [T, H, 128] in slot order
    assert (img - lay).abs().max().item() <= 1e-12 * lay.abs().max().item()
    assert torch.equal(G.head_slots(64), torch.arange(64))


def moved(ref, mut, bound):
    """largest displacement of a wrong variant in units of the per-element bound (where the bound is defined)."""
    m = bound > 0
    return ((mut - ref).abs()[m] / bound[m]).max().item()


def operand(t, dt=torch.float16):
    return t.to(dt).double()


def test_wrong_variants_move_the_output_past_ten_bounds():
    g = torch.Generator().manual_seed(6)
    R, C, B, H = 8, 33, 2, 2
    q = operand(torch.randn(R, C, B, H, 64, generator=g) / 8)
    k = operand(torch.randn(R, C, B, H, 64, generator=g))
    v = operand(torch.randn(R, C, B, H, 64, generator=g))
    # one score slice dropped: the softmax of the remaining partial maps
    parts, _ = G.row_scores(q, k, S=4)
    parts = parts.float()
    probs, pb = G.row_softmax(parts)
    assert moved(probs, G.row_softmax(parts, drop_slice=2)[0], pb) >= 10
    assert moved(G.row_scores(q, k, 4)[0], G.row_scores(q, k, 4, drop_slice=1)[0], G.row_scores(q, k, 4)[1]) >= 10
    # ctx_R / ctx_C swapped in the context store
    ctx, cb = G.row_context(probs.half().double(), v)
    cb = G.store(ctx, cb, torch.float16)
    E = H * 64
    assert moved(G.ctx_layout(ctx, E), G.ctx_layout(ctx, E, swap=True), G.ctx_layout(cb, E)) >= 10
    # the row map transposed
    xr = torch.randn(B * R * C, 64, generator=g, dtype=torch.float64)
    y, yb = G.dense(operand(torch.randn(B * C * R, 64, generator=g)), operand(torch.randn(64, 64, generator=g)))
    ref, rb = G.resid_rowmap(xr, y, yb, B, R, C)
    assert moved(ref, G.resid_rowmap(xr, y, yb, B, R, C, transpose=True)[0], rb) >= 10
    # the ESM-2 key permutation applied to the MSA vt_rows layout
    vs = v.permute(2, 0, 1, 3, 4).reshape(B * R, C, H, 64)
    vb = G.store(vs, G.acc_bound(vs.abs(), 768), torch.float16)
    Cp = 64
    assert moved(G.vt_rows_layout(vs, B, R, Cp), G.vt_rows_layout(vs, B, R, Cp, perm=True),
                 G.vt_rows_layout(vb, B, R, Cp)) >= 10
    # the two 64-column slices of a 128-wide head swapped; row_pos shifted by one
    T, Hh, K = 40, 2, 256
    x = operand(torch.randn(T, K, generator=g))
    w = operand(torch.randn(Hh * 128, K, generator=g) / 16)
    inv_freq = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    cos, sin = G.rope_tables(inv_freq, T + 1)
    y, by = G.dense(x, w)
    pos = torch.arange(T)
    qv, qb = G.rope(y.view(T, Hh, 128), by.view(T, Hh, 128), cos, sin, pos)
    qb = G.store(qv, qb, torch.float16)
    lay, lb = G.qk_layout(qv[None]), G.qk_layout(qb[None])
    assert moved(lay, G.qk_layout(qv[None], swap_halves=True), lb) >= 10
    shifted, _ = G.rope(y.view(T, Hh, 128), by.view(T, Hh, 128), cos, sin, pos + 1)
    assert moved(lay, G.qk_layout(shifted[None]), lb) >= 10


def test_row_score_slices_restates_the_engine():
    # engine_msa.hip row_score_slices: 12 heads, one 256-tile map per head -> up to 8 slices while S tiles <= 256 + 6
    assert G.row_score_slices(1, 12, 64, 256) == 8
    assert G.row_score_slices(1, 12, 30, 256) == 6
    assert G.row_score_slices(1, 12, 7, 1024) == 1     # 192 tiles: a second slice would pass 256 + 96
    assert G.row_score_slices(2, 12, 64, 257) == 2
    assert G.row_score_slices(1, 12, 1, 1) == 1
