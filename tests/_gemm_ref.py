"""fp64 reference of the generalised GEMM forms of the persistent kernel (gemm8_kernel<..., GEN = true>) and of the tied
row-attention softmax, stated as the operations of the model, with a per-element error bound.

Arithmetic and layout are kept apart.  The model-level functions work on the axes of oracle/msa_oracle.py (MSA tensors
[R, C, B, ...], einsums of axial_attention.py) and of esm/rotary_embedding.py; the ``*_layout`` functions then scatter a
model-level result into the output layout the kernel documents (kernels.h, gemm_epi.h) by the index formula written
there.  A stride convention that kernel and reference both got wrong cannot then agree by accident.

Inputs are the kernel's own operand values (already rounded to fp16 / bf16, cos / sin fp32 tables as passed).  Every
function returns (value fp64, bound fp64) with ``|kernel - value| <= bound`` per element:
  * accumulation: ACC_C * gamma_{K+1} * sum_k |a_k w_k| (+ |bias|): products of fp16 / bf16 values are exact in fp32, the
    K products and the bias are summed in fp32 in some order; ACC_C = 2 allows an MFMA adder that truncates instead of
    rounding to nearest;
  * the epilogue's own fp32 operations: a few u of the magnitudes they combine;
  * a store in the operand dtype: half an ulp of the result (``store``).

Mutation knobs (the CPU suite shows each moves the output by >= 10x the bound): ``drop_slice`` (row_scores / row_softmax),
``swap`` (ctx_layout: ctx_R and ctx_C exchanged), ``transpose`` (rowmap_rows), ``perm`` (vt_rows_layout with the ESM-2
key permutation), ``swap_halves`` (qk_layout of 128-wide heads), position offsets (rope: pass shifted positions)."""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff
ACC_C = 2.0
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: U}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}


def gamma(n):
    return n * U / (1 - n * U)


def acc_bound(mag, K):
    return ACC_C * gamma(K + 1) * mag


def store(y, b, dtype):
    """Bound after the result is rounded to `dtype` (round to nearest: half an ulp, plus the subnormal spacing)."""
    return b + UNIT[dtype] * (y.abs() + b) + TINY[dtype]


def dense(a, w, bias=None):
    """nn.Linear: y[..., n] = sum_k a[..., k] w[n, k] + bias[n]."""
    a, w = a.double(), w.double()
    y, mag = a @ w.T, a.abs() @ w.abs().T
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return y, acc_bound(mag, a.shape[-1])


def scale(y, b, s):
    """y * s with s an fp32 scalar (the epilogue's q scale times row_keep): one more rounding."""
    s = float(torch.tensor(s, dtype=torch.float32))
    v = y * s
    return v, abs(s) * b + U * v.abs()


def rope(y, b, cos, sin, pos):
    """esm/rotary_embedding.py:11-20 on [..., T, H, d] (natural dim order, dim i pairs with i + d/2): x cos + rotate_half(x)
    sin with cos / sin [*, d/2] fp32 tables indexed by the positions `pos` [T].  The epilogue forms
    y1 = fma(a1, c, -(a2 s)), y2 = fma(a2, c, a1 s): 2 roundings each."""
    h = y.shape[-1] // 2
    c, s = cos.double()[pos], sin.double()[pos]
    c, s = torch.cat((c, c), -1)[:, None], torch.cat((s, s), -1)[:, None]
    rot = torch.cat((-y[..., h:], y[..., :h]), -1)
    rb = torch.cat((b[..., h:], b[..., :h]), -1)
    rot_abs = torch.cat((y[..., h:], y[..., :h]), -1).abs()
    v = y * c + rot * s
    return v, c.abs() * b + s.abs() * rb + 3 * U * (y.abs() * c.abs() + rot_abs * s.abs())


# ---------------------------------------------------------------------------------------------------------------------
# model-level forms (axial_attention.py; msa_oracle.row_attention / column_attention)
# ---------------------------------------------------------------------------------------------------------------------
def rows_of(x):
    """[R, C, B, D] -> the engine's row order (b, r, c): [B R C, D]."""
    R, C, B, D = x.shape
    return x.permute(2, 0, 1, 3).reshape(B * R * C, D)


def from_rows(t, R, C, B):
    """inverse of rows_of."""
    return t.reshape(B, R, C, -1).permute(1, 2, 0, 3)


def col_rows_of(x):
    """[R, C, B, D] -> the column-attention row order (b, c, r)."""
    R, C, B, D = x.shape
    return x.permute(2, 1, 0, 3).reshape(B * C * R, D)


def msa_proj(x, w, bias, heads, keep=None, sc=1.0):
    """q / k / v of axial_attention.py:82-88 on x [R, C, B, D]: F.linear(x, w, bias) * sc, times keep [B, R, C] (1 - pad)
    for q; cos / sin are the unit tables (MSA rows carry no rotary embedding).  -> [R, C, B, H, d]."""
    R, C, B, D = x.shape
    y, b = dense(x, w, bias)
    y, b = y.view(R, C, B, heads, -1), b.view(R, C, B, heads, -1)
    if sc != 1.0 or keep is not None:
        y, b = scale(y, b, sc)
        if keep is not None:
            k = keep.double().permute(1, 2, 0)[..., None, None]
            y, b = y * k, b * k
    return y, b


def row_scores(q, k, S=1, drop_slice=None):
    """axial_attention.py:90 ``einsum("rinhd,rjnhd->hnij", q, k)`` cut into S slices of R / S rows: [S, H, B, C, C]
    partial maps (the engine's tied-score GEMM, row_score_slices)."""
    R = q.shape[0]
    Rs = R // S
    q, k = q.double(), k.double()
    v, mag = [], []
    for s in range(S):
        qs, ks = q[s * Rs:(s + 1) * Rs], k[s * Rs:(s + 1) * Rs]
        v.append(torch.einsum("rinhd,rjnhd->hnij", qs, ks))
        mag.append(torch.einsum("rinhd,rjnhd->hnij", qs.abs(), ks.abs()))
    v, mag = torch.stack(v), torch.stack(mag)
    if drop_slice is not None:
        v[drop_slice] = 0
    return v, acc_bound(mag, Rs * q.shape[-1])


def row_softmax(parts, pad0=None, drop_slice=None):
    """axial_attention.py:96-100,127 on the S partial maps [S, H, B, C, C] (fp32, as the GEMM left them): summed, keys
    padded in MSA row 0 (pad0 [B, C] bool) filled with -10000, softmax over j.  -> probs [H, B, C, C].
    Bound: the fp32 sum of S parts (gamma_S), the shift and exp (4 u (1 + |s - max|) + 2 u), the fp32 sum over C keys
    and the division (gamma_{C+2}); relative errors of p_j add those of p_j's own exponent and of the normaliser."""
    p = parts.double()
    if drop_slice is not None:
        p = p.clone()
        p[drop_slice] = 0
    S = p.shape[0]
    s = p.sum(0)
    ds = gamma(S) * p.abs().sum(0)
    if pad0 is not None:
        m = pad0[None, :, None, :].expand_as(s)
        s = s.masked_fill(m, -10000.0)
        ds = ds.masked_fill(m, 0.0)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    probs = e / e.sum(-1, keepdim=True)
    rel = ds + 4 * U * (1 + (s - mx).abs()) + 2 * U
    rel_norm = (rel * probs).sum(-1, keepdim=True) + gamma(s.shape[-1] + 2)
    return probs, 2 * probs * (rel + rel_norm)


def row_context(probs, v):
    """axial_attention.py:111 ``einsum("hnij,rjnhd->rinhd", probs, v)``: [H, B, C, C] x [R, C, B, H, d] -> [R, C, B, H, d].
    The kernel contracts over Cp >= C keys, the padding holding zero probabilities."""
    p, v = probs.double(), v.double()
    y = torch.einsum("hnij,rjnhd->rinhd", p, v)
    mag = torch.einsum("hnij,rjnhd->rinhd", p.abs(), v.abs())
    Cp = (p.shape[-1] + 63) // 64 * 64
    return y, acc_bound(mag, Cp)


def column_attention_core(q, k, v):
    """axial_attention.py:207,217-218 without padding: [R, C, B, H, d] each -> ctx [R, C, B, H, d] (plain fp64; the
    flash kernel that computes it in the engine has tests of its own)."""
    w = torch.einsum("icnhd,jcnhd->hcnij", q.double(), k.double())
    return torch.einsum("hcnij,jcnhd->icnhd", w.softmax(-1), v.double())


def rowmap_rows(B, R, C, transpose=False):
    """out row of GEMM row m for the column-attention out-proj (remap_row, gemm_epi.h): GEMM rows are ordered (b, c, r),
    the residual stream (b, r, c).  -> index tensor [B C R]."""
    if transpose:
        R, C = C, R
    m = torch.arange(B * R * C)
    b, rem = m // (R * C), m % (R * C)
    c, r = rem // R, rem % R
    return (b * R + r) * C + c


def resid_rowmap(x_rows, y, by, B, R, C, transpose=False):
    """x[perm] += y: out-proj rows y (b, c, r) added to the residual rows (b, r, c); bound = that of y plus the fp32 add."""
    idx = rowmap_rows(B, R, C, transpose).to(x_rows.device)
    out, bnd = x_rows.double().clone(), torch.zeros_like(x_rows, dtype=torch.float64)
    out[idx] += y
    bnd[idx] = by + U * out[idx].abs()
    return out, bnd


# ---------------------------------------------------------------------------------------------------------------------
# kernel layouts (gemm_epi.h, kernels.h); each scatters a model-level tensor into the documented output buffer
# ---------------------------------------------------------------------------------------------------------------------
def permute_keys16(T):
    """slot of key t in the ESM-2 V^T layout: inside each group of 16 the 4-groups 1 and 2 are swapped."""
    t = torch.arange(T)
    t16 = t & 15
    return (t & ~15) | (((t16 >> 2) & 1) << 3) | (((t16 >> 3) & 1) << 2) | (t16 & 3)


def head_slots(d):
    """slot of natural dim i inside a head (elementwise.hip head_pad_index): identity for 64; for 128 the QKV epilogue's
    slice order dims [0,32) | [64,96) | [32,64) | [96,128), i.e. slice sl holds dims 32 sl .. 32 sl + 31 and their
    rotary partners 64 further up."""
    i = torch.arange(d)
    if d != 128:
        return i
    half, j = i >> 6, i & 63
    return (j >> 5) * 64 + half * 32 + (j & 31)


def qk_layout(t, swap_halves=False):
    """q / k [Bseq, T, H, d] (natural dims) -> [Bseq, H, T, d] in slot order (EPI_QKV_ROPE's head-major store)."""
    d = t.shape[-1]
    slots = head_slots(d)
    if swap_halves:
        slots = (slots + 64) % 128
    out = torch.empty_like(t.permute(0, 2, 1, 3))
    out[..., slots.to(t.device)] = t.permute(0, 2, 1, 3)
    return out


def weight_image(w, heads):
    """q or k weight rows [H d, K] (natural order) -> the packed image the QKV epilogue expects: row slot s of head h
    holds natural row i with head_slots(i) = s."""
    d = w.shape[0] // heads
    img = torch.empty_like(w).view(heads, d, -1)
    img[:, head_slots(d).to(w.device)] = w.view(heads, d, -1)
    return img.view_as(w)


def vt_esm2_layout(v, Tp):
    """v [Bseq, T, H, d] -> [Bseq, H, d, Tp], key t at slot permute_keys16(t) (EPI_V_T, vt_rows = 0); pad slots 0."""
    Bs, T, H, d = v.shape
    out = torch.zeros(Bs, H, d, Tp, dtype=v.dtype, device=v.device)
    out[..., permute_keys16(T).to(v.device)] = v.permute(0, 2, 3, 1)
    return out


def vt_rows_layout(v, B, R, Tp, perm=False):
    """v [B R, T, H, 64] (sequences (b, r)) -> [B, H, R, 64, Tp] with keys in plain order (EPI_V_T with vt_rows = R)."""
    BR, T, H, d = v.shape
    out = torch.zeros(B, H, R, d, Tp, dtype=v.dtype, device=v.device)
    slots = (permute_keys16(T) if perm else torch.arange(T)).to(v.device)
    out[..., slots] = v.view(B, R, T, H, d).permute(0, 3, 1, 4, 2)
    return out


def scores_layout(parts, Cp):
    """[S, H, B, C, C] partial maps -> [B, S, H, C, Cp] (batch entry zo = b S + s, zi = h; row stride ldc = Cp); the
    columns [C, Cp) are left 0 here (the kernel's are unspecified)."""
    S, H, B, C, _ = parts.shape
    out = torch.zeros(B, S, H, C, Cp, dtype=parts.dtype, device=parts.device)
    out[..., :C] = parts.permute(2, 0, 1, 3, 4)
    return out


def ctx_layout(ctx, ldc, swap=False):
    """row-attention context [R, C, B, H, 64] -> the flat EPI_MSA_CTX buffer:
    out[((zo ctx_R + r) ctx_C + i) ldc + zi 64 + d] with zo = b, zi = h, ctx_R = R, ctx_C = C (kernels.h)."""
    R, C, B, H, d = ctx.shape
    cR, cC = (C, R) if swap else (R, C)
    r, i, b, h, e = torch.meshgrid(*(torch.arange(n, device=ctx.device) for n in ctx.shape), indexing="ij")
    idx = ((b * cR + r) * cC + i) * ldc + h * 64 + e
    out = torch.zeros(B * R * C * ldc, dtype=ctx.dtype, device=ctx.device)
    out[idx.reshape(-1)] = ctx.reshape(-1)
    return out


def row_score_slices(B, H, R, C):
    """engine_msa.hip row_score_slices: the number of K slices the engine cuts the tied-score GEMM into."""
    tiles = B * H * ((C + 255) // 256) ** 2
    best = 1
    s = 2
    while s <= 8 and s * tiles <= 256 + tiles // 2:
        if R % s == 0:
            best = s
        s += 1
    return best


def rope_tables(inv_freq, n):
    """cos / sin [n, len(inv_freq)] fp32 (rotary_embedding.py:47-61, launch_rope_table)."""
    t = torch.arange(n, dtype=torch.float32)
    f = torch.outer(t, inv_freq.float())
    return f.cos(), f.sin()
