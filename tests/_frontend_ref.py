"""Plain CPU references of the token front end (csrc/elementwise.hip: seq_stats, packed_stats, zero_gap_rows, embed,
embed_esm1, add_positions, scale_rows, msa_embed, sinus_table, rope_table; csrc/scoring.hip: gather_rows), restated from
the reference's formulas and shared by tests/test_frontend_reference_cpu.py (which pins them to the oracles) and
tests/test_frontend_ops_gpu.py (which holds the kernels to them).

Bookkeeping is integer arithmetic.  Where the kernel does one or two IEEE fp32 operations in a fixed order with no
multiply-add that a compiler could contract, the reference does the same operations in torch fp32 on the CPU and the
result is bit-determined; elsewhere the reference is fp64 of the fp32 inputs and comes with a bound.
"""
import math

import torch

NEG_INF = float("-inf")
KEEP_TRAIN = 1 - 0.15 * 0.8  # esm2.py:90 / esm1.py:127: 1 - mask_ratio_train; torch multiplies by fp32(0.88)


def bits(t):
    """The bit patterns of an fp32 tensor (int32), for comparisons that tell +0 from -0 and one NaN from another."""
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32)


def same_bits(got, want):
    """Bit equality of two fp32 tensors, except that any NaN matches any NaN (0 / 0 has no specified sign or payload)."""
    g, w = got.cpu(), want.cpu()
    if g.shape != w.shape:
        return False
    nan = torch.isnan(w)
    return bool(torch.equal(torch.isnan(g), nan)) and bool(torch.equal(bits(g)[~nan], bits(w)[~nan]))


# ---- statistics ---------------------------------------------------------------------------------------------------------
def seq_stats_ref(tokens, pad_idx=1, mask_idx=32):
    """esm2.py:82 (padding_mask), :86-92 (mask_ratio_observed and its divisor), :108-109, multihead_attention.py:368-374.
    tokens int64 [B,T] -> scale fp32 [B] = 1 - n_mask.float() / n_nonpad.float() (one correctly rounded division of two
    exactly representable integers and one subtraction: the bits are fixed; 0 / 0 = NaN for a row of padding only),
    key_bias fp32 [B,T] = 0 / -inf, seq_info int32 [B,2] = (#pads, 1 + index of the last non-pad token, 0 if none), keep
    fp32 [B,T] = 1 - pad."""
    B, T = tokens.shape
    pad = tokens.eq(pad_idx)
    n_pad = pad.sum(-1)
    n_mask = tokens.eq(mask_idx).sum(-1)
    scale = 1.0 - n_mask.float() / (T - n_pad).float()
    key_bias = torch.zeros((B, T), dtype=torch.float32).masked_fill(pad, NEG_INF)
    idx = torch.arange(1, T + 1).expand(B, T)
    last = torch.where(pad, torch.zeros_like(idx), idx).amax(-1)
    seq_info = torch.stack([n_pad, last], -1).to(torch.int32)
    return scale, key_bias, seq_info, (~pad).float()


def packed_stats_ref(tokens, segments, pad_idx=1, mask_idx=32):
    """The same per segment of a packed row space (kernels.h, launch_packed_stats): tokens int64 [rows], segments [(first
    row, length)].  Returns scale_row, key_bias, keep fp32 [rows], row_pos int32 [rows], seg_npad int32 [n]; rows outside
    every segment are (1, -inf, 0, 0)."""
    rows = tokens.numel()
    scale_row = torch.ones(rows, dtype=torch.float32)
    key_bias = torch.full((rows,), NEG_INF, dtype=torch.float32)
    row_pos = torch.zeros(rows, dtype=torch.int32)
    keep = torch.zeros(rows, dtype=torch.float32)
    npad = []
    for start, n in segments:
        s, kb, info, kp = seq_stats_ref(tokens[start:start + n].view(1, n), pad_idx, mask_idx)
        scale_row[start:start + n] = s[0]
        key_bias[start:start + n] = kb[0]
        keep[start:start + n] = kp[0]
        row_pos[start:start + n] = torch.arange(n, dtype=torch.int32)
        npad.append(int(info[0, 0]))
    return scale_row, key_bias, row_pos, torch.tensor(npad, dtype=torch.int32), keep


def gap_rows(segments, rows):
    """bool [rows]: the rows outside every segment."""
    gap = torch.ones(rows, dtype=torch.bool)
    for start, n in segments:
        gap[start:start + n] = False
    return gap


# ---- embeddings ---------------------------------------------------------------------------------------------------------
def gather_table(tokens, table):
    """table[tok], a zero row for a token outside [0, vocab) (the kernels' guard `tok >= 0 && tok < vocab`)."""
    ok = (tokens >= 0) & (tokens < table.shape[0])
    return table[tokens.clamp(0, table.shape[0] - 1)].masked_fill(~ok.unsqueeze(-1), 0.0)


def embed_ref(tokens, table, scale, pad_idx=1, mask_idx=32, token_dropout=True):
    """esm2.py:84 (gather), :87 (zero <mask> rows), :92 as (x * fp32(0.88)) / scale — a multiplication and a division, no
    addition a compiler could contract: the bits are fixed — and :94-95 (pad rows := +0).  tokens int64 [B,T], table fp32
    [vocab,E], scale fp32 [B] -> fp32 [B,T,E]."""
    x = gather_table(tokens, table)
    if token_dropout:
        x = x.masked_fill(tokens.eq(mask_idx).unsqueeze(-1), 0.0)
        x = (x * torch.tensor(KEEP_TRAIN, dtype=torch.float32)) / scale.view(-1, 1, 1)
    return x.masked_fill(tokens.eq(pad_idx).unsqueeze(-1), 0.0)


def embed_esm1_ref(tokens, table, scale, sinus, embed_scale, pad_idx=1, mask_idx=33, token_dropout=False):
    """esm1.py:123 (embed_scale * gather), :125-131 (token dropout), :133 (+ sinusoidal positions, the zero row for pads:
    modules.py:278-282,293-294) in fp64 from the fp32 inputs; no pad zeroing (that is ESM-1b, :135-139).  Returns (ref
    fp64 [B,T,E], bound [B,T,E]): bound = 3 * 2^-24 * (|embed_scale e| / |scale| + |pe|) — at most three roundings, each
    at most half an ulp of an intermediate no larger than that sum."""
    es = float(torch.tensor(embed_scale, dtype=torch.float32))
    e = gather_table(tokens, table).double() * es
    mag = e.abs()
    if token_dropout:
        e = e.masked_fill(tokens.eq(mask_idx).unsqueeze(-1), 0.0)
        mag = e.abs() / scale.double().abs().view(-1, 1, 1)
        e = e * float(torch.tensor(KEEP_TRAIN, dtype=torch.float32)) / scale.double().view(-1, 1, 1)
    T = tokens.shape[1]
    pe = sinus[:T].double().unsqueeze(0) * tokens.ne(pad_idx).unsqueeze(-1).double()
    return e + pe, 3 * 2.0 ** -24 * (mag + pe.abs())


def embed_esm1_pad_rows_ref(tokens, table, scale, embed_scale, mask_idx=33, token_dropout=False):
    """What embed_esm1 leaves on a <pad> row — the scaled embedding and no position term — in the kernel's fp32 operations
    (a multiplication, then with token dropout a multiplication and a division; no addition): the bits are fixed.  fp32
    [B,T,E], meaningful on pad rows."""
    x = gather_table(tokens, table) * torch.tensor(embed_scale, dtype=torch.float32)
    if token_dropout:
        x = x.masked_fill(tokens.eq(mask_idx).unsqueeze(-1), 0.0)
        x = (x * torch.tensor(KEEP_TRAIN, dtype=torch.float32)) / scale.view(-1, 1, 1)
    return x


def position_ids(tokens, pad_idx=1):
    """LearnedPositionalEmbedding.forward (modules.py:247-248): cumsum(nonpad) * nonpad + padding_idx, int64 [.., T]."""
    m = tokens.ne(pad_idx).long()
    return torch.cumsum(m, dim=-1) * m + pad_idx


def add_positions_ref(x, tokens, pos_emb, pad_idx=1):
    """esm1.py:133 / modules.py:240-257: x + pos_emb[position] — one fp32 addition per element: the bits are fixed.  tokens
    [B,T], x fp32 [B,T,E]; the index is clamped to the table as in the kernel (never reached inside the length rule)."""
    return x + pos_emb[position_ids(tokens, pad_idx).clamp_max(pos_emb.shape[0] - 1)]


def add_positions_packed_ref(x, tokens, pos_emb, segments, pad_idx=1):
    """The same per segment of a packed row space: tokens [rows], x [rows,E]; rows outside every segment keep their value."""
    out = x.clone()
    for start, n in segments:
        out[start:start + n] = add_positions_ref(x[start:start + n][None], tokens[start:start + n][None], pos_emb, pad_idx)[0]
    return out


def msa_embed_ref(tokens, tok_emb, pos_emb, msa_pos=None, pad_idx=1):
    """msa_transformer.py:152-165: x = (embed_tokens[tok] + embed_positions[position]) + msa_position_embedding[r] — two
    fp32 additions in that order: the bits are fixed.  tokens int64 [B,R,C].  Returns x fp32 [B,R,C,D], keep fp32 [B,R,C]
    = 1 - pad (:171-172), col_fill fp32 [B,C,R] = pad (the column-attention key mask, axial_attention.py:211-215, in the
    (b,c)-major layout), any_pad (bool: :153-155)."""
    B, R, C = tokens.shape
    x = gather_table(tokens, tok_emb) + pos_emb[position_ids(tokens, pad_idx).clamp_max(pos_emb.shape[0] - 1)]
    if msa_pos is not None:
        x = x + msa_pos.reshape(-1, tok_emb.shape[1])[:R].view(1, R, 1, -1)
    pad = tokens.eq(pad_idx)
    return x, (~pad).float(), pad.transpose(1, 2).float().contiguous(), bool(pad.any())


# ---- position tables ----------------------------------------------------------------------------------------------------
def rope_inv_freq(dim):
    """rotary_embedding.py:40."""
    return 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))


def sinus_freq(half):
    """SinusoidalPositionalEmbedding.get_embedding, modules.py:285-287."""
    return torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))


def angles32(freq, T, pos0=0):
    """fp32 [T, half]: fp32(pos0 + t) * freq[i] — one fp32 multiplication: the bits are fixed (modules.py:288,
    rotary_embedding.py:54-55)."""
    return torch.arange(pos0, pos0 + T, dtype=torch.float32).unsqueeze(1) * freq.float().unsqueeze(0)


def sinus_table_ref(freq, T, pos0):
    """fp64 [T, 2 half]: sin | cos (modules.py:289) of the fp32 angle."""
    a = angles32(freq, T, pos0).double()
    return torch.cat([torch.sin(a), torch.cos(a)], dim=1)


def rope_table_ref(inv_freq, T):
    """(cos, sin) fp64 [T, half] of the fp32 angle (rotary_embedding.py:58-59 without the duplicated half)."""
    a = angles32(inv_freq, T).double()
    return torch.cos(a), torch.sin(a)


TABLE_BOUND = 2.0 ** -22  # 4 fp32 ulp at 1.0: precise sinf / cosf are a few ulp, the fast hardware path ~1e-4 at 1000 rad


# ---- row gather ---------------------------------------------------------------------------------------------------------
def gather_rows_ref(x, sel):
    """x[clamp(sel, 0, N - 1)] (kernels.h, launch_gather_rows)."""
    return x[sel.long().clamp(0, x.shape[0] - 1)]
