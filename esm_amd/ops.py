"""Thin torch-tensor wrappers over the single-kernel entry points of libesmk.so.

Used by the parity tests and micro-benchmarks; the model path (esm_amd.esm2.ESM2) calls
``esmk_forward`` directly.  Every function requires CUDA (HIP) tensors and launches on the
current stream; nothing here falls back to torch math.
"""
import ctypes

import torch

from . import _native as N
from .packing import ragged_views


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("esm_amd.ops: tensors must be contiguous")


def layernorm(x, gamma, beta, operand_dtype=torch.float16, want_op=True, want_f32=False, variant=None):
    """torch.nn.LayerNorm(E, eps=1e-5) on fp32 rows (reference esm/modules.py:68-81).  variant: None or 7 = the engine's
    kernel form, 0 = the plain one-row-per-wave form (tests)."""
    _req_cuda(x, gamma, beta)
    assert x.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    rows, E = x.reshape(-1, x.shape[-1]).shape
    y = torch.empty_like(x, dtype=operand_dtype) if want_op else None
    y32 = torch.empty_like(x) if want_f32 else None
    code = N.dtype_code(operand_dtype) | (0 if variant is None else (variant + 1) << 8)
    N.check(N.lib.esmk_op_layernorm(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(y32), rows, E,
                                    code, N.cur_stream()))
    return y, y32


def masked_row_mean(x, counts, first_row=1):
    """out[b] = x[b, first_row : first_row + counts[b]].mean(0) in fp32 (reference scripts/extract.py:113-116);
    x [B,T,E] fp32 / fp16 / bf16, counts int32 [B] on the same device.  Empty slices give NaN, as torch.mean."""
    _req_cuda(x, counts)
    assert x.dim() == 3 and counts.dtype == torch.int32 and counts.numel() == x.shape[0]
    B, T, E = x.shape
    out = torch.empty((B, E), dtype=torch.float32, device=x.device)
    N.check(N.lib.esmk_op_masked_row_mean(N.ptr(x), N.dtype_code(x.dtype), N.ptr(counts), N.ptr(out), B, T, E,
                                          first_row, N.cur_stream()))
    return out


def linear(a, w, bias=None, epilogue=N.EPI_STORE_T, out=None, force_generic=False, force_old=False,
           panel_c=0, half_m=0):
    """nn.Linear with fused epilogue: a [M,K], w [N,K] (both f16 or bf16), bias fp32 [N]."""
    _req_cuda(a, w, bias, out)
    assert a.dtype == w.dtype and a.dtype in (torch.float16, torch.bfloat16)
    M, K = a.shape
    Nn, K2 = w.shape
    assert K == K2
    if epilogue == N.EPI_RESID_F32:
        assert out is not None and out.dtype == torch.float32 and tuple(out.shape) == (M, Nn)
    elif out is None:
        odt = a.dtype if epilogue in (N.EPI_STORE_T, N.EPI_GELU_T) else torch.float32
        out = torch.empty((M, Nn), dtype=odt, device=a.device)
    # 0x100: generic 64x64 kernel, 0x200: one-tile-per-workgroup 256x256 kernel (gemm.hip) instead of the
    # persistent kernel (gemm8.hip); bits 20..27: tile-order panel width of the persistent kernel
    code = (N.dtype_code(a.dtype) | (0x100 if force_generic else 0) | (0x200 if force_old else 0) | (panel_c << 20)
            | ({0: 0, 1: 1, -1: 2}[half_m] << 28))  # half_m: 1 force 128-row tiles, -1 never
    N.check(N.lib.esmk_op_linear(N.ptr(a), N.ptr(w), N.ptr(bias), N.ptr(out), M, Nn, K, epilogue, code,
                                 N.cur_stream()))
    return out


def split_weight(w):
    """w [N,K] (fp32 / fp16 / bf16) -> fp16 [N,2K]: 64-column K tiles interleaved hi | lo, hi = fp16(w), lo = fp16(w - hi)
    (the weight image of the f16x2 precision mode)."""
    _req_cuda(w)
    Nn, K = w.shape
    out = torch.zeros((Nn, 2 * K), dtype=torch.float16, device=w.device)
    N.check(N.lib.esmk_op_split_weight(N.ptr(w.contiguous()), N.dtype_code(w.dtype), N.ptr(out), Nn, K, N.cur_stream()))
    return out


def linear_split(a, w2, bias=None, epilogue=N.EPI_STORE_T, out=None):
    """a [M,K] fp16, w2 = split_weight(w) [N,2K]: a . (w_hi + w_lo)^T + bias with the epilogues of ``linear``."""
    _req_cuda(a, w2, bias, out)
    assert a.dtype == torch.float16 and w2.dtype == torch.float16
    M, K = a.shape
    Nn = w2.shape[0]
    assert w2.shape[1] == 2 * K
    if epilogue == N.EPI_RESID_F32:
        assert out is not None and out.dtype == torch.float32 and tuple(out.shape) == (M, Nn)
    elif out is None:
        out = torch.empty((M, Nn), dtype=torch.float16 if epilogue in (N.EPI_STORE_T, N.EPI_GELU_T) else torch.float32,
                          device=a.device)
    N.check(N.lib.esmk_op_linear_split(N.ptr(a), N.ptr(w2), N.ptr(bias), N.ptr(out), M, Nn, K, epilogue, N.cur_stream()))
    return out


def linear_f32(a, w, bias=None, gelu=False, out=None, M=None):
    """The exact-fp32 MFMA linear of the LM head (esmk_op_linear_f32): a fp32 [M,lda] (the first K columns are read), w fp32
    [N,K], bias fp32 [N] or None -> act(a . w^T + bias) written into out fp32 [>= M, ldc >= N] (allocated [M,N] when None;
    only the [M,N] corner is written)."""
    _req_cuda(a, w, bias, out)
    assert a.dtype == w.dtype == torch.float32 and a.dim() == w.dim() == 2
    Nn, K = w.shape
    M = a.shape[0] if M is None else M
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=a.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] >= M and a.shape[0] >= M
    N.check(N.lib.esmk_op_linear_f32(N.ptr(a), a.shape[1], N.ptr(w), N.ptr(bias), N.ptr(out), out.shape[1], M, Nn, K,
                                     int(bool(gelu)), N.cur_stream()))
    return out


def layernorm_ex(x, gamma, beta, y=None, y32=None, operand_dtype=torch.float16, row_keep=None, map_R=0, map_C=0, x3=False,
                 eps=1e-5, variant=None):
    """Every form of the LayerNorm launch (esmk_op_layernorm_ex): x fp32 [rows,E] -> y (operand dtype, [>= rows, ldy]: its
    row stride is taken from the tensor) and / or y32 fp32 [>= rows, E], both the caller's and written in place.  row_keep
    fp32 [rows] scales the output rows; map_R / map_C write input row (b,r,c) to output row (b,c,r); x3: y rows hi | hi | lo
    per 64 columns (fp16, ldy >= 3 E)."""
    _req_cuda(x, gamma, beta, y, y32, row_keep)
    assert x.dtype == torch.float32 and x.dim() == 2 and gamma.dtype == beta.dtype == torch.float32
    rows, E = x.shape
    assert y is None or (y.dim() == 2 and y.dtype == operand_dtype and y.shape[0] >= rows)
    assert y32 is None or (y32.dtype == torch.float32 and tuple(y32.shape[1:]) == (E,) and y32.shape[0] >= rows)
    assert row_keep is None or (row_keep.dtype == torch.float32 and row_keep.numel() == rows)
    code = N.dtype_code(operand_dtype) | (0 if variant is None else (variant + 1) << 8)
    N.check(N.lib.esmk_op_layernorm_ex(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(y32), rows, E, code,
                                       N.ptr(row_keep), map_R, map_C, 0 if y is None else y.shape[1], int(bool(x3)),
                                       float(eps), N.cur_stream()))
    return y, y32


def split_weight_ex(w, dst, dst_ld, parts, row_map=False, col_map=False, head_dim=64):
    """The weight images of the precision modes (esmk_op_split_weight_ex): w [rows,cols] (fp32 / fp16 / bf16) into the
    caller's dst, rows of parts * dst_ld elements: parts 1 = conversion to dst.dtype, 2 = hi | lo, 3 = hi | lo | hi per
    64-column K tile (fp16).  row_map / col_map spread heads of head_dim over 64 slots (128: the q / k slice order); slots
    in between are left as they are."""
    _req_cuda(w, dst)
    rows, cols = w.shape
    N.check(N.lib.esmk_op_split_weight_ex(N.ptr(w), N.dtype_code(w.dtype), N.ptr(dst), N.dtype_code(dst.dtype), rows, cols,
                                          dst_ld, parts, int(bool(row_map)), int(bool(col_map)), head_dim, N.cur_stream()))
    return dst


def linear_gelu_x3(a3, w3, bias, out3=None, M=None):
    """fc1 + GELU of the f16x3 mode (esmk_op_linear_gelu_x3): a3 fp16 [M,K3] rows hi | hi | lo, w3 fp16 [N,K3] rows
    hi | lo | hi, bias fp32 [N] -> out3 fp16 [>= M, 3N] (allocated when None), gelu(a . w^T + bias) as hi | hi | lo."""
    _req_cuda(a3, w3, bias, out3)
    assert a3.dtype == w3.dtype == torch.float16 and bias is not None and bias.dtype == torch.float32
    M = a3.shape[0] if M is None else M
    Nn, K3 = w3.shape
    assert a3.shape[1] == K3 and a3.shape[0] >= M
    if out3 is None:
        out3 = torch.empty((M, 3 * Nn), dtype=torch.float16, device=a3.device)
    assert out3.dtype == torch.float16 and out3.shape[1] == 3 * Nn and out3.shape[0] >= M
    N.check(N.lib.esmk_op_linear_gelu_x3(N.ptr(a3), N.ptr(w3), N.ptr(bias), N.ptr(out3), M, Nn, K3, N.cur_stream()))
    return out3


LOG2E = 1.4426950408889634


def to_log2_domain(q, dtype=None):
    """The attention kernels take q with log2(e) folded in (the engine's QKV epilogue does that in fp32 before the
    single rounding to the operand dtype).  Returns (q_kernel, q_effective): the operand-dtype tensor to hand to the
    kernels and the fp32 natural-domain q it represents exactly (q_kernel / log2 e) — what a reference must use."""
    qk = (q.float() * LOG2E).to(dtype or q.dtype)
    return qk, qk.float() / LOG2E


def attention(q, k, vt, key_bias=None, want_lse=False, seq_info=None, fill_any_pad=None, x3=False):
    """softmax(q k^T + key_bias) v.  q [B,H,T,D] in the LOG2 domain (``to_log2_domain``), k [B,H,T,D], D = 64 or 128
    (taken from q); vt [B,H,D,Tp] (layout of the fused QKV epilogue, see csrc/attention.hip).  Returns ctx
    [B*T, H*D] (+ the row log-sum-exp converted to the natural log, [B,H,T]).

    seq_info: int32 [B,2] = (#pads, 1 + index of the last non-pad token), the padded-batch form esmk_forward launches
    (needs key_bias).  fill_any_pad: int32 device tensor of one element — the MSA column form: key_bias holds 0/1
    fill flags, used when the flag is non-zero (D = 64).  x3: the f16x3 form, ctx [B*T, 3*H*64] with hi | hi | lo per
    head (D = 64, fp16).  Without any of the three this is esmk_op_attention (D = 64) or the plain d128 kernel."""
    _req_cuda(q, k, vt, key_bias, seq_info, fill_any_pad)
    B, H, T, D = q.shape
    assert vt.shape[-2] == D and vt.shape[-1] % 64 == 0 and vt.shape[-1] >= T
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device) if want_lse else None
    mode = 2 if x3 else 1 if fill_any_pad is not None else 0
    if seq_info is None and mode == 0 and D == 64 and vt.shape[-1] == (T + 63) // 64 * 64:
        ctx = torch.empty((B * T, H * 64), dtype=q.dtype, device=q.device)
        N.check(N.lib.esmk_op_attention(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), N.ptr(ctx), N.ptr(lse),
                                        B, H, T, N.dtype_code(q.dtype), N.cur_stream()))
    else:
        if seq_info is not None:
            assert seq_info.dtype == torch.int32 and tuple(seq_info.shape) == (B, 2)
        if fill_any_pad is not None:
            assert fill_any_pad.dtype == torch.int32 and fill_any_pad.numel() == 1
        ctx = torch.empty((B * T, H * D * (3 if x3 else 1)), dtype=q.dtype, device=q.device)
        N.check(N.lib.esmk_op_attention_ex(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), N.ptr(seq_info),
                                           N.ptr(fill_any_pad), N.ptr(ctx), N.ptr(lse), B, H, T, vt.shape[-1], D, mode,
                                           N.dtype_code(q.dtype), N.cur_stream()))
    return (ctx, lse / LOG2E) if want_lse else ctx  # the kernel's lse is log2-domain


def attention_biaskv(q, k, vt, bias_k, bias_v, key_bias=None, seq_info=None):
    """``attention`` (D = 64, padded-batch form) with the learned null key / value pair of the ESM-1 models: bias_k, bias_v
    [H,64] in the operand dtype (bias_k unscaled); T + 1 keys per row, the extra one never masked.  Returns ctx [B*T, H*64]
    and the natural-log row log-sum-exp [B,H,T], both INCLUDING the null key."""
    _req_cuda(q, k, vt, bias_k, bias_v, key_bias, seq_info)
    B, H, T, D = q.shape
    assert D == 64 and vt.shape[-2] == 64 and vt.shape[-1] % 64 == 0 and vt.shape[-1] >= T
    assert tuple(bias_k.shape) == (H, 64) and tuple(bias_v.shape) == (H, 64) and bias_k.dtype == bias_v.dtype == q.dtype
    assert bias_k.is_contiguous() and bias_v.is_contiguous()
    if seq_info is not None:
        assert seq_info.dtype == torch.int32 and tuple(seq_info.shape) == (B, 2)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    ctx = torch.empty((B * T, H * 64), dtype=q.dtype, device=q.device)
    N.check(N.lib.esmk_op_attention_biaskv(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), N.ptr(seq_info), N.ptr(bias_k),
                                           N.ptr(bias_v), N.ptr(ctx), N.ptr(lse), B, H, T, vt.shape[-1],
                                           N.dtype_code(q.dtype), N.cur_stream()))
    return ctx, lse / LOG2E


def attention_probs(q, k, lse, key_bias=None, out=None, layer=0, num_layers=1, fill_any_pad=None, msa_C=0,
                    out_dtype=torch.float32):
    """q in the log2 domain; lse: natural-log row log-sum-exp as returned by ``attention(..., want_lse=True)``.
    Maps [B, num_layers, H, T, T] (slice `layer`) in out_dtype (fp32 or q's dtype), D = 64 or 128 from q.  msa_C > 0:
    the MSA column layout [B / msa_C, num_layers, H, msa_C, T, T] with key_bias = fill flags and fill_any_pad as in
    ``attention`` (D = 64, fp32)."""
    _req_cuda(q, k, lse, key_bias, out, fill_any_pad)
    lse = (lse * LOG2E).contiguous()
    B, H, T, D = q.shape
    if out is None:
        shape = (B // msa_C, num_layers, H, msa_C, T, T) if msa_C else (B, num_layers, H, T, T)
        out = torch.empty(shape, dtype=out_dtype, device=q.device)
    assert out.dtype == out_dtype
    if D == 64 and msa_C == 0 and fill_any_pad is None and out_dtype == torch.float32:
        N.check(N.lib.esmk_op_attention_probs(N.ptr(q), N.ptr(k), N.ptr(lse), N.ptr(key_bias), N.ptr(out), B, H, T,
                                              layer, num_layers, N.dtype_code(q.dtype), N.cur_stream()))
    else:
        N.check(N.lib.esmk_op_attention_probs_ex(N.ptr(q), N.ptr(k), N.ptr(lse), N.ptr(key_bias), N.ptr(fill_any_pad),
                                                 N.ptr(out), B, H, T, D, layer, num_layers, msa_C,
                                                 N.dtype_code(out_dtype), N.dtype_code(q.dtype), N.cur_stream()))
    return out


def _segments_arg(segments):
    seg = torch.as_tensor(segments, dtype=torch.int32).reshape(-1, 2).contiguous().cpu()
    return seg, ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))


def attention_packed(q, k, vt, segments, key_bias=None, want_lse=False, bias_k=None, bias_v=None):
    """The attention core of a token-packed batch (esmk_op_attention_packed): q, k [H,rows,D] (q in the LOG2 domain),
    vt [H,D,Tp] with Tp >= rows + 64 (``make_vt_packed``), segments [n,2] = (first row, length) with starts at multiples
    of 16, key_bias fp32 [rows] (0 / -inf) or None.  Returns ctx [rows, H*D] — rows outside every segment are zero here
    (the kernel does not write them) — and, with want_lse, the natural-log row log-sum-exp [H,rows]."""
    _req_cuda(q, k, vt, key_bias)
    H, rows, D = q.shape
    seg, seg_ptr = _segments_arg(segments)
    ctx = torch.zeros((rows, H * D), dtype=q.dtype, device=q.device)
    lse = torch.zeros((H, rows), dtype=torch.float32, device=q.device) if want_lse else None
    N.check(N.lib.esmk_op_attention_packed(N.ptr(q), N.ptr(k), N.ptr(vt), N.ptr(key_bias), seg_ptr, seg.shape[0], rows,
                                           vt.shape[-1], H, D, N.dtype_code(q.dtype), N.ptr(bias_k), N.ptr(bias_v),
                                           N.ptr(ctx), N.ptr(lse), N.cur_stream()))
    return (ctx, lse / LOG2E) if want_lse else ctx


def attention_probs_packed(q, k, lse, segments, key_bias=None, layer=0, num_layers=1, out_dtype=torch.float32, out=None):
    """The attention maps of a token-packed batch (esmk_op_attention_probs_packed): q, k, segments, key_bias as in
    ``attention_packed``, lse the natural-log [H,rows] it returned.  Returns (flat, views): the ragged buffer and, per
    segment, its [num_layers, H, len, len] view (slice `layer` is written)."""
    _req_cuda(q, k, lse, key_bias, out)
    H, rows, D = q.shape
    seg, seg_ptr = _segments_arg(segments)
    lens = seg[:, 1].tolist()
    if out is None:
        out = torch.zeros((num_layers * H * sum(n * n for n in lens),), dtype=out_dtype, device=q.device)
    assert out.dtype == out_dtype
    lse2 = (lse * LOG2E).contiguous()
    N.check(N.lib.esmk_op_attention_probs_packed(N.ptr(q), N.ptr(k), N.ptr(lse2), N.ptr(key_bias), seg_ptr, seg.shape[0],
                                                 rows, H, D, num_layers, layer, N.dtype_code(q.dtype),
                                                 int(out_dtype != torch.float32), N.ptr(out), out.numel(), N.cur_stream()))
    return out, ragged_views(out, lens, (num_layers, H))


def make_vt_packed(v):
    """v [H,rows,D] of a packed row space -> vt [H,D,rows + 64]: ``make_vt``'s layout plus the spare (zero) key tile the
    packed attention kernel may read behind the last row."""
    H, rows, D = v.shape
    assert rows % 64 == 0
    vt = torch.zeros((H, D, rows + 64), dtype=v.dtype, device=v.device)
    vt[:, :, :rows] = make_vt(v[None])[0]
    return vt


def contacts(attn, tokens, w, b, eos_idx=2, prepend_bos=True, append_eos=True):
    """ContactPredictionHead.forward (reference esm/modules.py:338-357)."""
    _req_cuda(attn, tokens, w, b)
    B, L, H, T, _ = attn.shape
    C = L * H
    S = T - int(prepend_bos) - int(append_eos)
    scratch = torch.empty((B * C * (S + 1),), dtype=torch.float32, device=attn.device)
    out = torch.empty((B, S, S), dtype=torch.float32, device=attn.device)
    N.check(N.lib.esmk_op_contacts(N.ptr(attn), N.ptr(tokens), N.ptr(w.reshape(-1)), N.ptr(b.reshape(-1)),
                                   N.ptr(scratch), N.ptr(out), B, C, T, eos_idx, int(prepend_bos),
                                   int(append_eos), N.cur_stream()))
    return out


def contacts_fused(q, k, lse, tokens, w, b=None, key_bias=None, segments=None, pad_idx=1, eos_idx=2,
                   prepend_bos=True, append_eos=True, head_groups=0, workspace=None, out=None):
    """Contact maps of predict_contacts through the fused kernels (csrc/contacts.hip), the layers' q, k and lse given.

    Padded: q, k [L,B,H,T,D], lse [L,B,H,T], key_bias fp32 [B,T] (0 / -inf) or None, tokens int64 [B,T] -> [B,S,S].
    Packed: segments = int32 [n_seg,2] (first row, length) on the host; q, k [L,H,rows,D], lse [L,H,rows], key_bias
    [rows], tokens [rows] -> the ragged fp32 buffer (each segment with S > 0, in table order, flattened).
    q in the LOG2 domain (``to_log2_domain``); lse the NATURAL-log row log-sum-exp (as ``attention`` returns it),
    converted here as fp32(lse * log2 e) in fp64.  w fp32 [L*H], b fp32 [1].  head_groups: 0 = the engine's choice.
    workspace: optional uint8 buffer of at least the queried size (a caller may pre-fill it).
    Returns (maps, head groups used)."""
    _req_cuda(q, k, tokens, w, b, key_bias, workspace, out)
    D = q.shape[-1]
    assert q.dtype == k.dtype and q.shape == k.shape and tokens.dtype == torch.int64
    lse2 = (lse.double() * LOG2E).float().contiguous()
    L = q.shape[0]
    bos, eos = int(prepend_bos), int(append_eos)
    if segments is None:
        _, B, H, T, _ = q.shape
        seg_p, n_seg = None, 0
        n_out = B * (T - bos - eos) ** 2
    else:
        _, H, T, _ = q.shape
        B = 1
        seg = torch.as_tensor(segments, dtype=torch.int32).reshape(-1, 2).contiguous().cpu()
        n_seg = seg.shape[0]
        seg_p = ctypes.cast(seg.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        n_out = sum(max(int(n) - bos - eos, 0) ** 2 for n in seg[:, 1].tolist())
    assert lse2.numel() == q.numel() // D
    n = ctypes.c_size_t()
    N.check(N.lib.esmk_op_contacts_fused_workspace_bytes_ex(B, H, T, L, D, seg_p, n_seg, bos, eos, head_groups,
                                                           ctypes.byref(n)))
    if workspace is None:
        workspace = torch.empty(max(n.value, 1), dtype=torch.uint8, device=q.device)
    assert workspace.numel() >= n.value
    if out is None:
        out = torch.empty(n_out, dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.numel() >= n_out
    used = ctypes.c_int(0)
    N.check(N.lib.esmk_op_contacts_fused_ex(N.ptr(q), N.ptr(k), N.ptr(lse2), N.ptr(key_bias), N.ptr(tokens),
                                            N.ptr(w.reshape(-1)), N.ptr(b), seg_p, n_seg, N.ptr(out),
                                            N.ptr(workspace), workspace.numel(), B, H, T, L, D, pad_idx, eos_idx, bos,
                                            eos, head_groups, ctypes.byref(used), N.dtype_code(q.dtype),
                                            N.cur_stream()))
    if segments is None:
        S = T - bos - eos
        out = out[:n_out].view(B, S, S)
    return out, used.value


_GEMM_EX_PTRS = ("A", "W", "bias", "out", "q", "k", "vt", "cos", "sin", "row_keep", "row_pos")


def gemm_ex(epilogue, **fields):
    """One launch of the persistent GEMM with generalised addressing (esmk_op_gemm_ex, include/esmk.h): keyword
    arguments are the fields of esmk_gemm_ex_args.  Pointer fields take GPU tensors (any view: the address of its first
    element) or None; A decides the operand dtype.  Nothing is allocated: every output buffer is the caller's."""
    a = N.EsmkGemmExArgs()
    a.size = ctypes.sizeof(a)
    a.batch, a.batch_inner, a.head_dim, a.scaling = 1, 1, 64, 1.0
    a.epilogue = epilogue
    a.operand_dtype = N.dtype_code(fields["A"].dtype)
    for name, v in fields.items():
        if name in _GEMM_EX_PTRS:
            if v is not None and not v.is_cuda:
                raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
            setattr(a, name, v.data_ptr() if v is not None else None)
        else:
            setattr(a, name, v)
    N.check(N.lib.esmk_op_gemm_ex(ctypes.byref(a), N.cur_stream()))


def msa_row_softmax(scores, keep, any_pad, probs, B, H, R, C, ldp, nslice=1, attn_out=None, layer=0, num_layers=1):
    """Tied row-attention softmax (esmk_op_msa_row_softmax): scores fp32 [B, nslice, H, C, ldp], keep fp32 [B, R, C],
    any_pad int32 [1] on the GPU -> probs (operand dtype, [B, H, C, ldp]) and optionally attn_out fp32
    [B, num_layers, H, C, C] slice `layer`."""
    _req_cuda(scores, keep, any_pad, probs, attn_out)
    assert scores.dtype == torch.float32 and keep.dtype == torch.float32 and any_pad.dtype == torch.int32
    N.check(N.lib.esmk_op_msa_row_softmax(N.ptr(scores), N.ptr(keep), N.ptr(any_pad), N.ptr(probs), N.ptr(attn_out),
                                          B, H, R, C, ldp, layer, num_layers, nslice, N.dtype_code(probs.dtype),
                                          N.cur_stream()))
    return probs


def permute_keys16(t):
    """Key position used by the V^T layout: inside each group of 16 keys the 4-groups 1 and 2
    are swapped (position p holds key perm[p])."""
    idx = torch.arange(t)
    t16 = idx & 15
    pos = (idx & ~15) | (((t16 >> 2) & 1) << 3) | (((t16 >> 3) & 1) << 2) | (t16 & 3)
    return pos


def make_vt(v):
    """Reference layout helper: v [B,H,T,D] -> vt [B,H,D,Tp] as the QKV epilogue writes it (D = 64 or 128: the key
    permutation is the same for both head dims, csrc/attention128.hip)."""
    B, H, T, D = v.shape
    Tp = (T + 63) // 64 * 64
    vt = torch.zeros((B, H, D, Tp), dtype=v.dtype, device=v.device)
    pos = permute_keys16(T).to(v.device)
    vt[:, :, :, pos] = v.transpose(2, 3)
    return vt


class QkvHandle:
    """Owns an esmk_model handle for the fused QKV + RoPE op (tests / micro-benchmarks)."""

    def __init__(self, embed_dim, num_heads, operand_dtype=torch.float16):
        cfg = N.EsmkConfig(1, embed_dim, num_heads, 4 * embed_dim, 33, 1, 32, 0, 2, 1, 1, 1,
                           N.dtype_code(operand_dtype))
        self.h = ctypes.c_void_p()
        N.check(N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        d = embed_dim // num_heads
        inv = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
        self.inv_freq = inv
        arr = (ctypes.c_float * inv.numel())(*inv.tolist())
        N.check(N.lib.esmk_set_rope_inv_freq(self.h, arr, inv.numel()))
        self.E, self.H, self.dtype = embed_dim, num_heads, operand_dtype

    def __call__(self, a, wqkv, bias, B, T, log2_domain=False):
        """log2_domain: q also carries log2(e) — the q ``attention`` / ``attention_probs`` take (esmk_op_qkv_rope2)."""
        _req_cuda(a, wqkv, bias)
        H, dev = self.H, a.device
        Tp = (T + 63) // 64 * 64
        q = torch.empty((B, H, T, 64), dtype=self.dtype, device=dev)
        k = torch.empty_like(q)
        vt = torch.empty((B, H, 64, Tp), dtype=self.dtype, device=dev)
        N.check(N.lib.esmk_op_qkv_rope2(self.h, N.ptr(a), N.ptr(wqkv), N.ptr(bias), N.ptr(q), N.ptr(k), N.ptr(vt),
                                        B, T, int(bool(log2_domain)), N.cur_stream()))
        return q, k, vt

    def __del__(self):
        if getattr(self, "h", None):
            N.lib.esmk_destroy(self.h)
            self.h = None


def mask_rows(tokens, positions, src_rows=None, mask_idx=32):
    """[n,T] int64: row i = tokens[src_rows[i]] (row 0 of [B,T] / the only row of [T] when ``src_rows`` is None) with
    position ``positions[i]`` set to ``mask_idx`` — the masked batch of the masked-marginal strategy (reference
    examples/variant-prediction/predict.py:208-209), built on the device.  positions / src_rows int32 [n]."""
    _req_cuda(tokens, positions, src_rows)
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and positions.dtype == torch.int32
    assert src_rows is None or (src_rows.dtype == torch.int32 and src_rows.numel() == positions.numel())
    B, T = tokens.shape
    n = positions.numel()
    out = torch.empty((n, T), dtype=torch.int64, device=tokens.device)
    N.check(N.lib.esmk_op_mask_rows(N.ptr(tokens), N.ptr(src_rows), N.ptr(positions), N.ptr(out), B, T, n, int(mask_idx),
                                    N.cur_stream()))
    return out


def log_softmax_rows(logits, target=None):
    """torch.log_softmax(logits, -1) of fp32 [n,V] rows, V <= 64 (one wavefront per row).  ``target`` int32 [n]: also returns
    the log-probability at that column of every row, the same bits as the gathered entry of the full output."""
    _req_cuda(logits, target)
    assert logits.dtype == torch.float32 and logits.dim() == 2
    assert target is None or (target.dtype == torch.int32 and target.numel() == logits.shape[0])
    n, V = logits.shape
    out = torch.empty_like(logits)
    tgt = torch.empty((n,), dtype=torch.float32, device=logits.device) if target is not None else None
    N.check(N.lib.esmk_op_log_softmax_rows(N.ptr(logits), N.ptr(out), N.ptr(target), N.ptr(tgt), n, V, N.cur_stream()))
    return out if target is None else (out, tgt)


def mask_rows_multi(tokens, pos_offsets, positions, src_rows=None, mask_idx=32):
    """[n,T] int64: row i = tokens[src_rows[i]] (row 0 / the only row when ``src_rows`` is None) with EVERY position of
    ``positions[pos_offsets[i] : pos_offsets[i + 1]]`` set to ``mask_idx`` — the joint mask of a multi-mutant variant.
    pos_offsets int32 [n + 1], positions int32 [total], src_rows int32 [n].  The lists are device data: offsets are clamped to
    [0, total] (a descending pair is an empty list: a plain copy), a position outside [0, T) masks nothing, a repeated
    position is harmless, a source row outside [0, B) is clamped."""
    _req_cuda(tokens, pos_offsets, positions, src_rows)
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    assert tokens.dtype == torch.int64 and tokens.dim() == 2
    assert pos_offsets.dtype == torch.int32 and pos_offsets.dim() == 1 and pos_offsets.numel() >= 2
    assert positions.dtype == torch.int32 and positions.dim() == 1
    n = pos_offsets.numel() - 1
    assert src_rows is None or (src_rows.dtype == torch.int32 and src_rows.numel() == n)
    B, T = tokens.shape
    total = positions.numel()
    if total == 0:  # nothing to mask anywhere; the entry still wants a pointer it will not read
        positions = torch.zeros((1,), dtype=torch.int32, device=tokens.device)
    out = torch.empty((n, T), dtype=torch.int64, device=tokens.device)
    N.check(N.lib.esmk_op_mask_rows_multi(N.ptr(tokens), N.ptr(src_rows), N.ptr(pos_offsets), N.ptr(positions), N.ptr(out),
                                          B, T, n, total, int(mask_idx), N.cur_stream()))
    return out


def score_rows(logprobs, wt, mt, var_offsets):
    """fp64 [n_var]: entry v = the sum over the rows r of ``var_offsets[v] : var_offsets[v + 1]``, ascending, of the fp32
    difference ``logprobs[r, mt[r]] - logprobs[r, wt[r]]``, added in fp64 by one lane per variant (a fixed order: no
    atomics).  logprobs fp32 [n_rows, V]; wt, mt int32 [n_rows] (clamped to [0, V)); var_offsets int32 [n_var + 1] (clamped
    to [0, n_rows]; an empty range gives 0.0)."""
    _req_cuda(logprobs, wt, mt, var_offsets)
    assert logprobs.dtype == torch.float32 and logprobs.dim() == 2
    n_rows, V = logprobs.shape
    assert wt.dtype == torch.int32 and mt.dtype == torch.int32 and wt.numel() == n_rows and mt.numel() == n_rows
    assert var_offsets.dtype == torch.int32 and var_offsets.dim() == 1 and var_offsets.numel() >= 2
    n_var = var_offsets.numel() - 1
    out = torch.empty((n_var,), dtype=torch.float64, device=logprobs.device)
    N.check(N.lib.esmk_op_score_rows(N.ptr(logprobs), N.ptr(wt), N.ptr(mt), N.ptr(var_offsets), N.ptr(out), n_rows, n_var, V,
                                     N.cur_stream()))
    return out


def mask_rows_packed(tokens, src_rows, seg_starts, seg_lens, pos_offsets, positions, rows, mask_idx=32, pad_idx=1, out=None):
    """[rows] int64, ONE packed row space: copy i = the first ``seg_lens[i]`` tokens of ``tokens[src_rows[i]]`` at
    ``out[seg_starts[i] : seg_starts[i] + seg_lens[i]]`` with every position of ``positions[pos_offsets[i] : pos_offsets[i + 1]]``
    set to ``mask_idx``; the gap behind the copy, up to ``seg_starts[i + 1]`` (``rows`` behind the last copy), is filled with
    ``pad_idx`` — the token stream ``esmk_forward_packed_rows`` takes.  src_rows, seg_starts, seg_lens int32 [n], pos_offsets
    int32 [n + 1], positions int32 [total], all device data: a source row outside [0, B) is clamped, a start to [0, rows], a
    length to [0, T] and to the rows left, offsets to [0, total] (a descending pair is an empty list), a position outside
    [0, length) masks nothing, a repeated position is harmless.  ``rows`` % 64 == 0.  ``out``: the caller's buffer of at least
    ``rows`` int64 (tests that look at the memory around it)."""
    _req_cuda(tokens, src_rows, seg_starts, seg_lens, pos_offsets, positions, out)
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    n = src_rows.numel()
    for t in (src_rows, seg_starts, seg_lens, pos_offsets, positions):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    assert n >= 1 and seg_starts.numel() == n and seg_lens.numel() == n and pos_offsets.numel() == n + 1
    B, T = tokens.shape
    total = positions.numel()
    if total == 0:  # nothing to mask anywhere; the entry still wants a pointer it will not read
        positions = torch.zeros((1,), dtype=torch.int32, device=tokens.device)
    if out is None:
        out = torch.empty((rows,), dtype=torch.int64, device=tokens.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= rows
    N.check(N.lib.esmk_op_mask_rows_packed(N.ptr(tokens), N.ptr(src_rows), N.ptr(seg_starts), N.ptr(seg_lens), N.ptr(pos_offsets),
                                           N.ptr(positions), N.ptr(out), B, T, n, total, int(rows), int(mask_idx), int(pad_idx),
                                           N.cur_stream()))
    return out


def sum_target_rows(logprobs, target, offsets):
    """fp64 [n_seq]: entry s = the sum over the rows r of ``offsets[s] : offsets[s + 1]``, ascending, of the fp32
    ``logprobs[r, target[r]]``, added in fp64 by one lane per sequence (a fixed order: no atomics).  logprobs fp32 [n_rows, V];
    target int32 [n_rows] (clamped to [0, V)); offsets int32 [n_seq + 1] (clamped to [0, n_rows]; an empty range gives 0.0)."""
    _req_cuda(logprobs, target, offsets)
    assert logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.is_contiguous()
    n_rows, V = logprobs.shape
    assert target.dtype == torch.int32 and target.numel() == n_rows
    assert offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2
    n_seq = offsets.numel() - 1
    out = torch.empty((n_seq,), dtype=torch.float64, device=logprobs.device)
    N.check(N.lib.esmk_op_sum_target_rows(N.ptr(logprobs), N.ptr(target), N.ptr(offsets), N.ptr(out), n_rows, n_seq, V,
                                          N.cur_stream()))
    return out


# ---- windows (include/esmk.h: esmk_op_window_rows, esmk_op_blend_rows, esmk_op_stitch_contacts; esm_amd/windows.py)
def window_rows(tokens, src_rows, starts, mask_offsets, mask_positions, Tw, head_tok=-1, tail_tok=-1, mask_idx=32):
    """[n,Tw] int64 window copies: copy i, column c = ``tokens[src_rows[i], starts[i] + c - h]`` (h = 1 if ``head_tok`` >= 0;
    row and column clamped into ``tokens``), column 0 = ``head_tok`` and column Tw - 1 = ``tail_tok`` where those are >= 0 (a
    wrapped window; both negative: a raw token slice).  ``mask_positions[mask_offsets[i] : mask_offsets[i + 1]]`` are token
    coordinates of the SOURCE row: an entry that lands on a body column of the copy becomes ``mask_idx``; one outside the
    copy's range or on an overridden column masks nothing; a repeated one is harmless.  src_rows, starts int32 [n],
    mask_offsets int32 [n + 1] (clamped to [0, total]; a descending pair is an empty list), mask_positions int32 [total]."""
    _req_cuda(tokens, src_rows, starts, mask_offsets, mask_positions)
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    assert tokens.dtype == torch.int64 and tokens.dim() == 2
    for t in (src_rows, starts, mask_offsets, mask_positions):
        assert t.dtype == torch.int32 and t.dim() == 1
    n = src_rows.numel()
    assert n >= 1 and starts.numel() == n and mask_offsets.numel() == n + 1
    B, T = tokens.shape
    total = mask_positions.numel()
    if total == 0:  # nothing to mask anywhere; the entry still wants a pointer it will not read
        mask_positions = torch.zeros((1,), dtype=torch.int32, device=tokens.device)
    out = torch.empty((n, int(Tw)), dtype=torch.int64, device=tokens.device)
    N.check(N.lib.esmk_op_window_rows(N.ptr(tokens), N.ptr(src_rows), N.ptr(starts), N.ptr(mask_offsets), N.ptr(mask_positions),
                                      N.ptr(out), B, T, n, int(Tw), total, int(head_tok), int(tail_tok), int(mask_idx),
                                      N.cur_stream()))
    return out


def blend_rows(x, offsets, src, weights):
    """fp32 [n_out,E]: row r = ``(sum_k weights[k] * x[src[k]]) / sum_k weights[k]`` over k in ``offsets[r] : offsets[r + 1]``,
    ascending, accumulated in fp32 by one lane per element (a fixed order: no atomics).  A list of one entry copies the row
    (converted to fp32) exactly, an empty list gives zeros.  x [N,E] fp32 / fp16 / bf16, E % 4 == 0; offsets int32 [n_out + 1]
    (clamped to [0, total]), src int32 [total] (clamped to [0, N)), weights fp32 [total], positive."""
    _req_cuda(x, offsets, src, weights)
    assert x.dim() == 2 and offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2
    assert src.dtype == torch.int32 and weights.dtype == torch.float32 and src.dim() == 1 and weights.numel() == src.numel()
    Nr, E = x.shape
    n_out = offsets.numel() - 1
    total = src.numel()
    if total == 0:  # every list is empty; the entry still wants pointers it will not read
        src = torch.zeros((1,), dtype=torch.int32, device=x.device)
        weights = torch.ones((1,), dtype=torch.float32, device=x.device)
    out = torch.empty((n_out, E), dtype=torch.float32, device=x.device)
    N.check(N.lib.esmk_op_blend_rows(N.ptr(x), N.dtype_code(x.dtype), N.ptr(offsets), N.ptr(src), N.ptr(weights), N.ptr(out), Nr,
                                     E, n_out, total, N.cur_stream()))
    return out


def stitch_contacts(maps, starts, Lb, body_lo=0):
    """fp32 [Lb,Lb]: entry (i, j) copied from the window of ``maps`` fp32 [n_w,R,R] that owns the pair — among the windows that
    hold both residues (window w covers ``starts[w] - body_lo`` .. + R - 1) the one with the least |2 s + R - 1 - (i + j)|, a tie
    going to the lower start; NaN where no window holds both.  starts int32 [n_w] on the device."""
    _req_cuda(maps, starts)
    assert maps.dtype == torch.float32 and maps.dim() == 3 and maps.shape[1] == maps.shape[2]
    assert starts.dtype == torch.int32 and starts.numel() == maps.shape[0]
    n_w, R, _ = maps.shape
    out = torch.empty((int(Lb), int(Lb)), dtype=torch.float32, device=maps.device)
    N.check(N.lib.esmk_op_stitch_contacts(N.ptr(maps), N.ptr(starts), N.ptr(out), n_w, R, int(Lb), int(body_lo), N.cur_stream()))
    return out


# ---- sampling (include/esmk.h: esmk_op_permute_positions, esmk_op_sample_rows[_ex], esmk_op_select_rows, esmk_op_commit_tokens)
def _seed64(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed} is outside [0, 2^64)")
    return seed


def permute_positions(pos_offsets, positions, chain_ids, seed=0, epoch=0):
    """int32 [total]: chain c's slice ``pos_offsets[c] : pos_offsets[c + 1]`` is a Fisher-Yates shuffle of the same slice of
    ``positions``, drawn from Philox counters (chain_ids[c], epoch, 0, i) under the key ``seed`` — it depends on nothing else,
    so a chain gets the same order alone and in any batch.  pos_offsets int32 [n_chain + 1] (clamped to [0, total]; a
    descending pair is an empty list), positions int32 [total], chain_ids int32 [n_chain], all on the device.  Elements outside
    every slice are zero."""
    _req_cuda(pos_offsets, positions, chain_ids)
    for t in (pos_offsets, positions, chain_ids):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    n_chain = chain_ids.numel()
    assert n_chain >= 1 and pos_offsets.numel() == n_chain + 1
    total = positions.numel()
    out = torch.zeros((total,), dtype=torch.int32, device=positions.device)
    if total == 0:
        return out
    N.check(N.lib.esmk_op_permute_positions(N.ptr(pos_offsets), N.ptr(positions), N.ptr(chain_ids), N.ptr(out), n_chain, total,
                                            _seed64(seed), int(epoch), N.cur_stream()))
    return out


def sample_rows(logprobs, row_chain, row_index, allowed_mask, inv_temperature=1.0, seed=0, step=0, exclude=None, want_u=True):
    """One token per row of ``logprobs`` fp32 [n, V] (V <= 64): ``(token int32 [n], logq fp32 [n], u fp32 [n] or None)``.
    The candidates of a row are the bits of the Python int ``allowed_mask`` below V, minus ``exclude[i]`` (int32 [n]; -1:
    none).  ``inv_temperature`` > 0: the inverse-CDF draw of include/esmk.h from softmax(logprobs * inv_temperature) over the
    candidates with the uniform of Philox counter (row_chain[i], step, 1, row_index[i]) under the key ``seed``; 0: the
    candidate with the largest log-probability (ties: the lowest index).  No candidate: token -1.  ``logq`` is the
    log-probability of the drawn token under the distribution it was drawn from."""
    return _sample_rows(logprobs, row_chain, row_index, allowed_mask, inv_temperature, seed, step, exclude, want_u)[:3]


SCORE_KINDS = {None: 0, "none": 0, "confidence": 1, "entropy": 2}  # score_kind of esmk_op_sample_rows_ex


def check_filters(top_k, top_p):
    """``(int top_k, float top_p)`` of esmk_op_sample_rows_ex, or ValueError: top_k in 0 .. 64 (0: off), top_p in (0, 1] (1: off)."""
    if int(top_k) != top_k or not 0 <= int(top_k) <= 64:
        raise ValueError(f"top_k {top_k!r} must be an integer in 0 .. 64 (0: no top-k filter)")
    top_p = float(top_p)
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p {top_p!r} must lie in (0, 1] (1: no nucleus filter)")
    return int(top_k), top_p


def _sample_rows(logprobs, row_chain, row_index, allowed_mask, inv_temperature, seed, step, exclude, want_u, filters=None):
    """The checks, the outputs and the call of ``sample_rows`` (``filters`` None: esmk_op_sample_rows) and of ``sample_rows_ex``
    (``filters`` = (top_k, top_p, score, want_kept): esmk_op_sample_rows_ex)."""
    _req_cuda(logprobs, row_chain, row_index, exclude)
    assert logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.is_contiguous()
    n, V = logprobs.shape
    for t in (row_chain, row_index) + ((exclude,) if exclude is not None else ()):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()
    allowed_mask = int(allowed_mask)
    if not 0 <= allowed_mask < 2 ** 64:
        raise ValueError("allowed_mask is a bitset over at most 64 vocabulary entries")
    if filters is not None:
        top_k, top_p = check_filters(*filters[:2])
        score, want_kept = filters[2:]
        if score not in SCORE_KINDS:
            raise ValueError(f"score {score!r}: None, 'confidence' or 'entropy'")
        kind = SCORE_KINDS[score]
    dev = logprobs.device
    token = torch.empty((n,), dtype=torch.int32, device=dev)
    logq = torch.empty((n,), dtype=torch.float32, device=dev)
    u = torch.empty((n,), dtype=torch.float32, device=dev) if want_u else None
    head = (N.ptr(logprobs), N.ptr(row_chain), N.ptr(row_index), N.ptr(exclude), allowed_mask, float(inv_temperature),
            _seed64(seed), int(step))
    if filters is None:
        N.check(N.lib.esmk_op_sample_rows(*head, N.ptr(token), N.ptr(logq), N.ptr(u), n, V, N.cur_stream()))
        return token, logq, u, None, None
    score_out = torch.empty((n,), dtype=torch.float32, device=dev) if kind else None
    kept = torch.empty((n,), dtype=torch.int64, device=dev) if want_kept else None
    N.check(N.lib.esmk_op_sample_rows_ex(*head, top_k, top_p, kind, N.ptr(token), N.ptr(logq), N.ptr(u), N.ptr(score_out),
                                         N.ptr(kept), n, V, N.cur_stream()))
    return token, logq, u, score_out, kept


def sample_rows_ex(logprobs, row_chain, row_index, allowed_mask, inv_temperature=1.0, seed=0, step=0, exclude=None, want_u=True,
                   top_k=0, top_p=1.0, score=None, want_kept=True):
    """``sample_rows`` behind a top-k / nucleus filter, with a per-row score: ``(token int32 [n], logq fp32 [n], u fp32 [n] or
    None, score fp32 [n] or None, kept int64 [n] or None)``.  The candidates are ranked by their fp32 log-probability (ties: the
    lower token; NaN last); rank r is kept when ``(top_k == 0 or r < top_k) and (top_p >= 1 or E_r < top_p * W)``, E_r the fp32
    sum of the weights ``expf(z - max z)`` of the ranks before r, W the sum of all (include/esmk.h); the best candidate is
    always kept, and the draw and ``logq`` are those of ``sample_rows`` over the kept set.  ``top_k=0, top_p=1.0``: no filter,
    the bits of ``sample_rows``.  ``score``: None, ``"confidence"`` (max log q) or ``"entropy"`` (sum q log q, the negative
    entropy), q = softmax(logprobs * inv_temperature) over the candidates before filtering (greedy: inv_temperature 1); -inf
    for a row without candidates.  ``kept``: the kept set of every row as the 64-bit pattern of an int64 (bit 63 is the sign)."""
    return _sample_rows(logprobs, row_chain, row_index, allowed_mask, inv_temperature, seed, step, exclude, want_u,
                        (top_k, top_p, score, want_kept))


def select_rows(score, row_offsets, sel_offsets, rest_offsets=None, n_sel=None, n_rest=0, sel_out=None, rest_out=None):
    """Per chain the rows of the largest score: ``(sel int32 [n_sel], rest int32 [n_rest] or None)``.  Chain c owns the rows
    ``row_offsets[c] : row_offsets[c + 1]`` of ``score`` fp32 [n] (offsets clamped to [0, n]; a descending pair is an empty
    list); ``sel[sel_offsets[c] : sel_offsets[c + 1]]`` receives the row indices of its best rows, best first (ties: the lower
    row; NaN below everything), at most as many as the chain has; ``rest[rest_offsets[c] : rest_offsets[c + 1]]`` the other rows
    in ascending order, at most as many as the slice holds.  All offsets int32 [n_chain + 1] on the device; the host never
    reads them, so it passes the lengths ``n_sel`` / ``n_rest`` of the outputs (or the outputs themselves: elements outside
    every slice are left as they are; fresh outputs are filled with -1)."""
    _req_cuda(score, row_offsets, sel_offsets, rest_offsets, sel_out, rest_out)
    assert score.dtype == torch.float32 and score.dim() == 1 and score.is_contiguous()
    n = score.numel()
    n_chain = row_offsets.numel() - 1
    assert n >= 1 and n_chain >= 1
    for t in (row_offsets, sel_offsets) + ((rest_offsets,) if rest_offsets is not None else ()):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n_chain + 1 and t.is_contiguous()
    dev = score.device
    if sel_out is None:
        sel_out = torch.full((int(n_sel),), -1, dtype=torch.int32, device=dev)
    if rest_out is None and rest_offsets is not None and int(n_rest) > 0:
        rest_out = torch.full((int(n_rest),), -1, dtype=torch.int32, device=dev)
    for t in (sel_out,) + ((rest_out,) if rest_out is not None else ()):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    assert sel_out.numel() >= 1
    N.check(N.lib.esmk_op_select_rows(N.ptr(score), N.ptr(row_offsets), N.ptr(sel_offsets),
                                      N.ptr(rest_offsets if rest_out is not None else None), N.ptr(sel_out), N.ptr(rest_out),
                                      n_chain, n, sel_out.numel(), rest_out.numel() if rest_out is not None else 0,
                                      N.cur_stream()))
    return sel_out, rest_out


def commit_tokens(tokens, slots, positions, token):
    """In place: ``tokens[slots[i], positions[i]] = token[i]`` on int64 [B, T]; slots, positions, token int32 [n] on the
    device.  A row with token < 0 or a position outside [0, T) writes nothing; a slot outside [0, B) is clamped.  The (slot,
    position) pairs must be distinct.  Returns ``tokens``."""
    _req_cuda(tokens, slots, positions, token)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    n = token.numel()
    for t in (slots, positions, token):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()
    B, T = tokens.shape
    if n == 0:
        return tokens
    N.check(N.lib.esmk_op_commit_tokens(N.ptr(tokens), N.ptr(slots), N.ptr(positions), N.ptr(token), n, B, T, N.cur_stream()))
    return tokens


# ---- Metropolis-Hastings design (include/esmk.h: esmk_op_propose_mutations ... esmk_op_hastings_rows) ---------------------------
CONTACT_LOSSES = {"pos": 0, "bce": 1}  # kind of esmk_op_contact_energy


def propose_mutations(tokens, pos_offsets, positions, chain_ids, allowed_mask, force_new=True, seed=0, step=0, slots=None):
    """The uniform single-site proposal of every chain: ``(site, old, token)`` int32 [n_chain] each.  Chain c reads the Philox
    words at counter (chain_ids[c], step, 2, 0) under the key ``seed``: the site is element ``mulhi32(word0, len_c)`` of its list
    ``positions[pos_offsets[c] : pos_offsets[c + 1]]``, ``old`` the token ``tokens[slots[c], site]`` (``slots`` None: row c), the
    proposed token the set bit number ``mulhi32(word1, n_cand)`` of the candidates — the bits of ``allowed_mask`` below V = 64,
    minus ``old`` with ``force_new``.  An empty list: (-1, -1, -1); no candidate: token -1.  Everything on the device."""
    _req_cuda(tokens, pos_offsets, positions, chain_ids, slots)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    for t in (pos_offsets, positions, chain_ids) + ((slots,) if slots is not None else ()):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()
    n_chain = chain_ids.numel()
    assert n_chain >= 1 and pos_offsets.numel() == n_chain + 1 and (slots is None or slots.numel() == n_chain)
    B, T = tokens.shape
    assert slots is not None or n_chain <= B
    allowed_mask = int(allowed_mask)
    if not 0 <= allowed_mask < 2 ** 64:
        raise ValueError("allowed_mask is a bitset over at most 64 vocabulary entries")
    total = positions.numel()
    if total == 0:  # every list is empty; the entry still wants a pointer it will not read
        positions = torch.zeros((1,), dtype=torch.int32, device=tokens.device)
    site, old, tok = (torch.empty((n_chain,), dtype=torch.int32, device=tokens.device) for _ in range(3))
    N.check(N.lib.esmk_op_propose_mutations(N.ptr(tokens), N.ptr(slots), N.ptr(pos_offsets), N.ptr(positions), N.ptr(chain_ids),
                                            allowed_mask, int(bool(force_new)), _seed64(seed), int(step), N.ptr(site), N.ptr(old),
                                            N.ptr(tok), n_chain, B, T, total, 64, N.cur_stream()))
    return site, old, tok


def contact_energy(contacts, target, min_sep=6, kind="pos"):
    """``(energy fp64 [B], count int32 [B])``: the cross-entropy between the probabilities ``contacts`` fp32 [B, S, S] and
    ``target`` uint8 [S, S] (0 = no contact, 1 = contact, 2 = ignore) over the pairs i < j with j - i >= ``min_sep`` and target
    != 2, p clamped to [2^-24, 1 - 2^-24], in fp64.  ``"pos"``: -mean of log p over the target contacts; ``"bce"``: -mean of
    y log p + (1 - y) log(1 - p) over the counted pairs.  The order of addition does not depend on B; no term: 0.0."""
    _req_cuda(contacts, target)
    assert contacts.dtype == torch.float32 and contacts.dim() == 3 and contacts.is_contiguous()
    B, S, S2 = contacts.shape
    assert S == S2 and target.dtype == torch.uint8 and tuple(target.shape) == (S, S) and target.is_contiguous()
    if kind not in CONTACT_LOSSES:
        raise ValueError(f"contact loss {kind!r}: one of {tuple(CONTACT_LOSSES)}")
    energy = torch.empty((B,), dtype=torch.float64, device=contacts.device)
    count = torch.empty((B,), dtype=torch.int32, device=contacts.device)
    N.check(N.lib.esmk_op_contact_energy(N.ptr(contacts), N.ptr(target), N.ptr(energy), N.ptr(count), B, S, int(min_sep),
                                         CONTACT_LOSSES[kind], N.cur_stream()))
    return energy, count


def mh_accept(tokens, site, tok, chain_ids, e_cur, e_contact=None, lp_sum=None, n_res=None, hastings=None, w_contact=1.0, w_lm=1.0,
              inv_temperature=1.0, seed=0, step=0, slots=None, e_contact_cur=None, e_lm_cur=None):
    """The Metropolis-Hastings test of every chain, in place on ``tokens`` int64 [B, T] and ``e_cur`` fp64 [n_chain]:
    ``(accepted uint8, u fp64, e_prop fp64)`` [n_chain] each.  E' = w_contact * e_contact + w_lm * -(lp_sum / n_res) (a missing
    term is 0); accept iff tok >= 0 and (a >= 0 or u < exp(a)) with a = -(E' - e_cur) * inv_temperature + hastings and u the
    24-bit uniform of Philox counter (chain_ids[c], step, 3, 0); ``inv_temperature=inf``: iff E' <= e_cur.  An accepted chain
    gets ``tokens[slots[c], site[c]] = tok[c]`` (``slots`` None: row c), ``e_cur = E'`` and its component energies in
    ``e_contact_cur`` / ``e_lm_cur`` where given."""
    return _mh_accept(tokens, site, tok, chain_ids, e_cur, e_contact, lp_sum, n_res, hastings, w_contact, w_lm, seed, step, slots,
                      e_contact_cur, e_lm_cur, inv_temperature=inv_temperature)


def _mh_accept(tokens, site, tok, chain_ids, e_cur, e_contact, lp_sum, n_res, hastings, w_contact, w_lm, seed, step, slots,
               e_contact_cur, e_lm_cur, inv_temperature=None, ex=None):
    """The tensor checks, the outputs and the call of ``mh_accept`` (a scalar ``inv_temperature``: esmk_op_mh_accept) and of
    ``mh_accept_ex`` (``ex`` = (inv_t, rung, e_extra, w_extra, e_extra_cur): esmk_op_mh_accept_ex)."""
    inv_t, rung, e_extra, w_extra, e_extra_cur = ex if ex is not None else (None,) * 5
    f64 = (e_cur, e_contact, lp_sum, hastings, e_extra, e_contact_cur, e_lm_cur, e_extra_cur)
    i32 = (site, tok, chain_ids, n_res, slots, rung)
    _req_cuda(tokens, inv_t, *f64, *i32)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    if ex is not None:
        assert inv_t.dtype == torch.float64 and inv_t.dim() == 1 and inv_t.numel() >= 1 and inv_t.is_contiguous()
    n_chain = chain_ids.numel()
    for t in f64:
        assert t is None or (t.dtype == torch.float64 and t.dim() == 1 and t.numel() == n_chain and t.is_contiguous())
    for t in i32:
        assert t is None or (t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n_chain and t.is_contiguous())
    B, T = tokens.shape
    assert n_chain >= 1 and (slots is not None or n_chain <= B) and (lp_sum is None or n_res is not None)
    dev = tokens.device
    accepted = torch.empty((n_chain,), dtype=torch.uint8, device=dev)
    u = torch.empty((n_chain,), dtype=torch.float64, device=dev)
    e_prop = torch.empty((n_chain,), dtype=torch.float64, device=dev)
    head = (N.ptr(tokens), N.ptr(slots), N.ptr(site), N.ptr(tok), N.ptr(chain_ids), N.ptr(e_contact), N.ptr(lp_sum), N.ptr(n_res),
            N.ptr(hastings))
    tail = (N.ptr(accepted), N.ptr(u), N.ptr(e_prop), n_chain, B, T, N.cur_stream())
    if ex is None:
        N.check(N.lib.esmk_op_mh_accept(*head, float(w_contact), float(w_lm), float(inv_temperature), _seed64(seed), int(step),
                                        N.ptr(e_cur), N.ptr(e_contact_cur), N.ptr(e_lm_cur), *tail))
    else:
        N.check(N.lib.esmk_op_mh_accept_ex(*head, N.ptr(e_extra), float(w_contact), float(w_lm), float(w_extra), N.ptr(inv_t),
                                           N.ptr(rung), inv_t.numel(), _seed64(seed), int(step), N.ptr(e_cur),
                                           N.ptr(e_contact_cur), N.ptr(e_lm_cur), N.ptr(e_extra_cur), *tail))
    return accepted, u, e_prop


def hastings_rows(logprobs, old, new, inv_t_prop=1.0):
    """fp64 [n]: ``float64(float32(inv_t_prop)) * (float64(logprobs[c, old[c]]) - float64(logprobs[c, new[c]]))`` — the log ratio of
    the reverse and the forward proposal of a draw from the row ``logprobs`` fp32 [n, V]; 0 where a token is outside [0, V)."""
    _req_cuda(logprobs, old, new)
    assert logprobs.dtype == torch.float32 and logprobs.dim() == 2 and logprobs.is_contiguous()
    n, V = logprobs.shape
    for t in (old, new):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()
    out = torch.empty((n,), dtype=torch.float64, device=logprobs.device)
    N.check(N.lib.esmk_op_hastings_rows(N.ptr(logprobs), N.ptr(old), N.ptr(new), float(inv_t_prop), N.ptr(out), n, V,
                                        N.cur_stream()))
    return out


# ---- the n-gram term and replica exchange (include/esmk.h: esmk_op_ngram_energy ... esmk_op_replica_swap) -----------------------
def ngram_energy(tokens, first, S, code, A, tables):
    """fp64 [B]: lm-design's n-gram term of every chain of ``tokens`` int64 [B, T], whose residues are the positions ``first`` ..
    ``first + S - 1``.  ``code`` int32 [V] maps a token to 0 .. A-1 or -1 (outside the alphabet: its windows are left out);
    ``tables`` is a dict order n (1 .. 4) -> fp64 [A^n] of positive background probabilities, all on the device.  Per order the KL
    divergence sum p log(p / q) over the distinct n-grams of the chain, p their frequency among its valid windows; the orders
    are added ascending.  The order of addition does not depend on B."""
    _req_cuda(tokens, code, *tables.values())
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    assert code.dtype == torch.int32 and code.dim() == 1 and code.is_contiguous()
    B, T = tokens.shape
    A = int(A)
    mask, ptrs = 0, [None] * 4
    for n, q in tables.items():
        n = int(n)
        if not 1 <= n <= 4:
            raise ValueError(f"n-gram order {n}: one of 1 .. 4")
        assert q.dtype == torch.float64 and q.dim() == 1 and q.numel() == A ** n and q.is_contiguous()
        mask |= 1 << (n - 1)
        ptrs[n - 1] = N.ptr(q)
    out = torch.empty((B,), dtype=torch.float64, device=tokens.device)
    N.check(N.lib.esmk_op_ngram_energy(N.ptr(tokens), N.ptr(code), *ptrs, mask, N.ptr(out), B, T, int(first), int(S),
                                       code.numel(), A, N.cur_stream()))
    return out


def mh_accept_ex(tokens, site, tok, chain_ids, e_cur, inv_t, rung=None, e_contact=None, lp_sum=None, n_res=None, hastings=None,
                 e_extra=None, w_contact=1.0, w_lm=1.0, w_extra=0.0, seed=0, step=0, slots=None, e_contact_cur=None, e_lm_cur=None,
                 e_extra_cur=None):
    """``mh_accept`` with a temperature per chain and a third energy term: chain c uses ``inv_t[rung[c]]`` (``inv_t`` fp64
    [n_rung] on the device, ``rung`` int32 [n_chain] clamped, None: entry 0) and E' = (w_contact * e_contact + w_lm * -(lp_sum /
    n_res)) + w_extra * e_extra (``e_extra`` None: the sum of two).  With ``e_extra`` None and one rung the bits of ``mh_accept``.
    An accepted chain also gets ``e_extra_cur = e_extra``."""
    return _mh_accept(tokens, site, tok, chain_ids, e_cur, e_contact, lp_sum, n_res, hastings, w_contact, w_lm, seed, step, slots,
                      e_contact_cur, e_lm_cur, ex=(inv_t, rung, e_extra, w_extra, e_extra_cur))


def replica_swap(rung, e_cur, inv_t, inv_t_host, ladder_ids, seed=0, round=0):
    """Swap round ``round`` of the ladders of K = ``inv_t.numel()`` consecutive chains, in place on ``rung`` int32 [n_ladder * K] (a
    permutation of 0 .. K-1 per ladder): ``(accepted uint8, u fp64)`` [n_ladder * K] each.  The chains at rungs k and k + 1, k % 2
    == round % 2, exchange their rungs iff a >= 0 or u < exp(a) with a = (inv_t[k] - inv_t[k+1]) * (e_cur[x] - e_cur[y]) and u the
    24-bit uniform of Philox counter (ladder_ids[l], round, 4, k); u is -1 for a chain without a partner in this round.
    ``inv_t_host``: the K values on the host (a sequence of floats), checked there: finite and not negative."""
    _req_cuda(rung, e_cur, inv_t, ladder_ids)
    K = inv_t.numel()
    assert inv_t.dtype == torch.float64 and inv_t.dim() == 1 and inv_t.is_contiguous() and K >= 1
    n_ladder = ladder_ids.numel()
    assert ladder_ids.dtype == torch.int32 and ladder_ids.dim() == 1 and ladder_ids.is_contiguous() and n_ladder >= 1
    assert rung.dtype == torch.int32 and rung.dim() == 1 and rung.numel() == n_ladder * K and rung.is_contiguous()
    assert e_cur.dtype == torch.float64 and e_cur.dim() == 1 and e_cur.numel() == n_ladder * K and e_cur.is_contiguous()
    host = [float(v) for v in inv_t_host]
    assert len(host) == K
    accepted = torch.empty((n_ladder * K,), dtype=torch.uint8, device=rung.device)
    u = torch.empty((n_ladder * K,), dtype=torch.float64, device=rung.device)
    N.check(N.lib.esmk_op_replica_swap(N.ptr(rung), N.ptr(e_cur), N.ptr(inv_t), (ctypes.c_double * K)(*host), N.ptr(ladder_ids),
                                       _seed64(seed), int(round), N.ptr(accepted), N.ptr(u), n_ladder, K, N.cur_stream()))
    return accepted, u


# ---- MSA row selection (include/esmk.h: esmk_op_msa_mismatch_rows ... esmk_op_rank_keys) --------------------------------------
def _msa_dims(msa, L):
    """(N, L, ld) of a device byte matrix uint8 [N, ld] of which the first ``L`` columns count (None: all)."""
    _req_cuda(msa)
    assert msa.dtype == torch.uint8 and msa.dim() == 2
    N, ld = msa.shape
    L = ld if L is None else int(L)
    if N < 1 or not 1 <= L <= ld:
        raise ValueError(f"msa: need at least one row and 1 <= L <= {ld} columns, got N = {N}, L = {L}")
    return N, L, ld


def msa_mismatch_rows(msa, query, L=None):
    """int32 [nq, N]: ``out[q, j]`` = the number of columns below ``L`` in which rows ``query[q]`` and j of ``msa`` uint8
    [N, ld] differ.  ``query`` int32 [nq] on the device; an index outside [0, N) is clamped.  Every byte value is legal."""
    N_, L, ld = _msa_dims(msa, L)
    _req_cuda(query)
    assert query.dtype == torch.int32 and query.dim() == 1 and query.numel() >= 1
    nq = query.numel()
    out = torch.empty((nq, N_), dtype=torch.int32, device=msa.device)
    N.check(N.lib.esmk_op_msa_mismatch_rows(N.ptr(msa), N_, L, ld, N.ptr(query), nq, N.ptr(out), N.cur_stream()))
    return out


def msa_neighbor_counts(msa, max_mismatch, L=None):
    """int32 [N]: ``count[i]`` = the number of rows j (i itself included) that differ from row i in at most ``max_mismatch`` of
    the first ``L`` columns of ``msa`` uint8 [N, ld].  A negative ``max_mismatch`` gives zeros."""
    N_, L, ld = _msa_dims(msa, L)
    out = torch.empty((N_,), dtype=torch.int32, device=msa.device)
    N.check(N.lib.esmk_op_msa_neighbor_counts(N.ptr(msa), N_, L, ld, int(max_mismatch), N.ptr(out), N.cur_stream()))
    return out


def msa_greedy_select(msa, num, first=0, mode=0, L=None):
    """int32 [num]: the greedy row pick of include/esmk.h in pick order: ``sel[0] = first``, then the not-yet-selected row with
    the largest (``mode`` 0) or smallest (``mode`` 1) integer sum of mismatches to the rows picked so far, ties to the lowest
    row.  All steps run on the device; the host reads nothing in between."""
    N_, L, ld = _msa_dims(msa, L)
    work = torch.empty((N_,), dtype=torch.int32, device=msa.device)
    sel = torch.empty((max(int(num), 1),), dtype=torch.int32, device=msa.device)
    N.check(N.lib.esmk_op_msa_greedy_select(N.ptr(msa), N_, L, ld, int(first), int(num), int(mode), N.ptr(work), N.ptr(sel),
                                            N.cur_stream()))
    return sel


def msa_race_keys(n, seed=0, subsample=0, counts=None, device=None):
    """fp64 [n]: ``key_i = -log(u_i) * counts[i]``, u_i the 24-bit uniform of Philox counter (subsample, 0, 2, i) under the key
    ``seed``; ``counts`` int32 [n] on the device or None (all ones).  u_i == 0 or a count <= 0 gives +inf."""
    if counts is not None:
        _req_cuda(counts)
        assert counts.dtype == torch.int32 and counts.dim() == 1 and counts.numel() == int(n)
        device = counts.device
    key = torch.empty((int(n),), dtype=torch.float64, device=device if device is not None else "cuda")
    N.check(N.lib.esmk_op_msa_race_keys(N.ptr(counts), int(n), _seed64(seed), int(subsample), N.ptr(key), N.cur_stream()))
    return key


def rank_keys(key):
    """int32 [n]: ``rank[i]`` = the number of keys that come before key i in ascending order (equal keys: the lower index first;
    NaN after everything): a permutation of 0 .. n - 1.  ``key`` fp64 [n] on the device."""
    _req_cuda(key)
    assert key.dtype == torch.float64 and key.dim() == 1 and key.numel() >= 1
    rank = torch.empty((key.numel(),), dtype=torch.int32, device=key.device)
    N.check(N.lib.esmk_op_rank_keys(N.ptr(key), N.ptr(rank), key.numel(), N.cur_stream()))
    return rank


# ---- the categorical Jacobian (include/esmk.h: esmk_op_substitute_rows ... esmk_op_apc) ------------------------------------
def substitute_rows(tokens, positions, tok, src_rows=None, vocab=33):
    """[n,T] int64: row i = tokens[src_rows[i]] (row 0 of [B,T] / the only row of [T] when ``src_rows`` is None) with position
    ``positions[i]`` set to ``tok[i]`` — the substituted copies of the categorical Jacobian, built on the device.  positions,
    tok, src_rows int32 [n], all device data: a source row outside [0, B) is clamped, a position outside [0, T) or a token
    outside [0, vocab) substitutes nothing."""
    _req_cuda(tokens, positions, tok, src_rows)
    tokens = tokens.view(1, -1) if tokens.dim() == 1 else tokens
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.is_contiguous()
    n = positions.numel()
    for t in (positions, tok) + ((src_rows,) if src_rows is not None else ()):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.numel() == n and t.is_contiguous()
    B, T = tokens.shape
    out = torch.empty((n, T), dtype=torch.int64, device=tokens.device)
    N.check(N.lib.esmk_op_substitute_rows(N.ptr(tokens), N.ptr(src_rows), N.ptr(positions), N.ptr(tok), N.ptr(out), B, T, n,
                                          int(vocab), N.cur_stream()))
    return out


def jacobian_scatter(logits, wt, cols, J, copy0=0):
    """In place: ``J.view(L * nA, L, nA)[copy0 + c, j, b] = logits[c * L + j, cols[b]] - wt[j, cols[b]]`` (fp32) for the
    ``logits.shape[0] // L`` copies of a chunk.  logits fp32 [n_copies * L, V], wt fp32 [L, V], cols int32 [nA] on the device
    (clamped to [0, V)), J fp32 [L, nA, L, nA].  Returns ``J``."""
    _req_cuda(logits, wt, cols, J)
    assert J.dtype == torch.float32 and J.dim() == 4 and J.is_contiguous()
    L, nA = J.shape[0], J.shape[1]
    assert tuple(J.shape) == (L, nA, L, nA)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    V = logits.shape[1]
    assert wt.dtype == torch.float32 and tuple(wt.shape) == (L, V) and wt.is_contiguous()
    assert cols.dtype == torch.int32 and cols.dim() == 1 and cols.numel() == nA and cols.is_contiguous()
    assert logits.shape[0] % L == 0
    n_copies, copy0 = logits.shape[0] // L, int(copy0)
    assert n_copies >= 1 and 0 <= copy0 and copy0 + n_copies <= L * nA, (copy0, n_copies, L * nA)
    out = ctypes.c_void_p(J.data_ptr() + copy0 * L * nA * 4)
    N.check(N.lib.esmk_op_jacobian_scatter(N.ptr(logits), N.ptr(wt), N.ptr(cols), out, n_copies, L, nA, V, N.cur_stream()))
    return J


def _jacobian_dims(J):
    assert J.dtype == torch.float32 and J.dim() == 4 and J.is_contiguous()
    L, nA = J.shape[0], J.shape[1]
    assert tuple(J.shape) == (L, nA, L, nA)
    return L, nA


def jacobian_center(J):
    """In place on fp32 [L, nA, L, nA]: the mean along each of the four axes removed, as four passes in the order b, j, a, i
    (last axis first); in every pass the mean is the fp64 sum of the fp32 line in ascending index order, divided by n, and
    every element becomes ``(float)((double)x - mean)``.  Returns ``J``."""
    _req_cuda(J)
    L, nA = _jacobian_dims(J)
    N.check(N.lib.esmk_op_jacobian_center(N.ptr(J), L, nA, N.cur_stream()))
    return J


def jacobian_contacts(Jc):
    """fp32 [L, L]: ``S[i, j] = sqrt(sum_ab (0.5 * (Jc[i, a, j, b] + Jc[j, b, i, a])) ** 2)``, the terms in fp64 in a fixed
    order, rounded to fp32 once; symmetric bit for bit.  Jc fp32 [L, nA, L, nA] (``jacobian_center``'s result)."""
    _req_cuda(Jc)
    L, nA = _jacobian_dims(Jc)
    S = torch.empty((L, L), dtype=torch.float32, device=Jc.device)
    N.check(N.lib.esmk_op_jacobian_contacts(N.ptr(Jc), N.ptr(S), L, nA, N.cur_stream()))
    return S


def apc(S):
    """In place on fp32 [L, L]: the diagonal set to zero, then ``S[i, j] - r_i * c_j / s`` with the row, column and total sums
    of S in fp64 (rounded to fp32 once; ``s == 0``: no correction), the diagonal zero again.  Returns ``S``."""
    _req_cuda(S)
    assert S.dtype == torch.float32 and S.dim() == 2 and S.shape[0] == S.shape[1] and S.is_contiguous()
    L = S.shape[0]
    work = torch.empty((2 * L + 1,), dtype=torch.float64, device=S.device)
    N.check(N.lib.esmk_op_apc(N.ptr(S), N.ptr(work), L, N.cur_stream()))
    return S


# ---- the token front end, one launch at a time (include/esmk.h: esmk_op_seq_stats ... esmk_op_gather_rows) -----------------
def _out(t, shape, dtype, device):
    """The caller's output buffer (checked), or a fresh one: callers that look at the memory behind an output pass their own."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req_cuda(t)
    n = 1
    for s in shape:
        n *= s
    assert t.dtype == dtype and t.numel() == n, (t.dtype, tuple(t.shape), shape)
    return t


def seq_stats(tokens, pad_idx=1, mask_idx=32, want_keep=True, scale=None, key_bias=None, seq_info=None, keep=None):
    """Per-sequence statistics of tokens int64 [B,T] (esmk_op_seq_stats): scale fp32 [B] = 1 - n_mask / n_nonpad, key_bias
    fp32 [B,T] = 0 / -inf, seq_info int32 [B,2] = (#pads, 1 + last non-pad index), keep fp32 [B,T] = 1 - pad (None without
    want_keep)."""
    _req_cuda(tokens)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2
    B, T = tokens.shape
    dev = tokens.device
    scale = _out(scale, (B,), torch.float32, dev)
    key_bias = _out(key_bias, (B, T), torch.float32, dev)
    seq_info = _out(seq_info, (B, 2), torch.int32, dev)
    keep = _out(keep, (B, T), torch.float32, dev) if want_keep else None
    N.check(N.lib.esmk_op_seq_stats(N.ptr(tokens), B, T, pad_idx, mask_idx, 1, N.ptr(scale), N.ptr(key_bias), N.ptr(seq_info),
                                    N.ptr(keep), N.cur_stream()))
    return scale, key_bias, seq_info, keep


def packed_stats(tokens, segments, pad_idx=1, mask_idx=32, want_keep=True, scale_row=None, key_bias=None, row_pos=None,
                 seg_npad=None, keep=None):
    """The same per segment of a packed row space (esmk_op_packed_stats): tokens int64 [rows], segments [n,2] = (first row,
    length) on the host -> scale_row, key_bias fp32 [rows], row_pos int32 [rows], seg_npad int32 [n], keep fp32 [rows] or
    None; rows outside every segment get (1, -inf, 0, 0)."""
    _req_cuda(tokens)
    assert tokens.dtype == torch.int64 and tokens.dim() == 1
    rows, dev = tokens.numel(), tokens.device
    seg, seg_ptr = _segments_arg(segments)
    scale_row = _out(scale_row, (rows,), torch.float32, dev)
    key_bias = _out(key_bias, (rows,), torch.float32, dev)
    row_pos = _out(row_pos, (rows,), torch.int32, dev)
    seg_npad = _out(seg_npad, (seg.shape[0],), torch.int32, dev)
    keep = _out(keep, (rows,), torch.float32, dev) if want_keep else None
    N.check(N.lib.esmk_op_packed_stats(N.ptr(tokens), seg_ptr, seg.shape[0], rows, pad_idx, mask_idx, N.ptr(scale_row),
                                       N.ptr(key_bias), N.ptr(row_pos), N.ptr(seg_npad), N.ptr(keep), N.cur_stream()))
    return scale_row, key_bias, row_pos, seg_npad, keep


def zero_gap_rows(buf, segments, rows, row_bytes):
    """Rows outside every segment of buf (any dtype, at least rows * row_bytes bytes, in place) := 0 (esmk_op_zero_gap_rows)."""
    _req_cuda(buf)
    assert buf.numel() * buf.element_size() >= rows * row_bytes
    seg, seg_ptr = _segments_arg(segments)
    N.check(N.lib.esmk_op_zero_gap_rows(N.ptr(buf), seg_ptr, seg.shape[0], rows, row_bytes, N.cur_stream()))
    return buf


def embed(tokens, table, scale=None, pad_idx=1, mask_idx=32, token_dropout=True, out=None):
    """ESM-2 / ESM-1b embedding (esmk_op_embed): tokens int64 [B,T], table fp32 [vocab,E], scale fp32 [B] (seq_stats; with
    T = 1 the per-row scale of packed_stats) -> fp32 [B,T,E]."""
    _req_cuda(tokens, table, scale)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and table.dtype == torch.float32 and table.dim() == 2
    B, T = tokens.shape
    vocab, E = table.shape
    assert scale is None or (scale.dtype == torch.float32 and scale.numel() == B)
    out = _out(out, (B, T, E), torch.float32, tokens.device)
    N.check(N.lib.esmk_op_embed(N.ptr(tokens), N.ptr(table), N.ptr(scale), N.ptr(out), B, T, E, vocab, pad_idx, mask_idx,
                                int(bool(token_dropout)), N.cur_stream()))
    return out


def embed_esm1(tokens, table, sinus, embed_scale, scale=None, pad_idx=1, mask_idx=32, token_dropout=False, out=None):
    """ESM-1 embedding (esmk_op_embed_esm1): embed_scale * table[tok], token dropout, + sinus[t] (fp32 [>= T, E]) on non-pad
    tokens -> fp32 [B,T,E]."""
    _req_cuda(tokens, table, sinus, scale)
    assert tokens.dtype == torch.int64 and tokens.dim() == 2 and table.dtype == sinus.dtype == torch.float32
    B, T = tokens.shape
    vocab, E = table.shape
    assert sinus.dim() == 2 and sinus.shape[0] >= T and sinus.shape[1] == E
    assert scale is None or (scale.dtype == torch.float32 and scale.numel() == B)
    out = _out(out, (B, T, E), torch.float32, tokens.device)
    N.check(N.lib.esmk_op_embed_esm1(N.ptr(tokens), N.ptr(table), N.ptr(scale), N.ptr(sinus), N.ptr(out), B, T, E, vocab,
                                     pad_idx, mask_idx, int(bool(token_dropout)), float(embed_scale), N.cur_stream()))
    return out


def add_positions(tokens, pos_emb, x, pad_idx=1, segments=None, longest=None):
    """x += the learned positions of ESM-1b (esmk_op_add_positions), in place.  Padded: tokens int64 [B,T], x fp32 [B,T,E].
    Packed: tokens [rows], x [rows,E], segments [n,2] on the host, longest = the longest segment (default: from the table)."""
    _req_cuda(tokens, pos_emb, x)
    assert tokens.dtype == torch.int64 and pos_emb.dtype == x.dtype == torch.float32 and pos_emb.dim() == 2
    npos, E = pos_emb.shape
    assert x.numel() == tokens.numel() * E
    if segments is None:
        B, T = tokens.shape
        N.check(N.lib.esmk_op_add_positions(N.ptr(tokens), N.ptr(pos_emb), N.ptr(x), B, T, E, pad_idx, npos, None, 0, 0,
                                            N.cur_stream()))
    else:
        seg, seg_ptr = _segments_arg(segments)
        T = int(seg[:, 1].max()) if longest is None else longest
        N.check(N.lib.esmk_op_add_positions(N.ptr(tokens), N.ptr(pos_emb), N.ptr(x), seg.shape[0], T, E, pad_idx, npos,
                                            seg_ptr, seg.shape[0], tokens.numel(), N.cur_stream()))
    return x


def scale_rows(x, keep):
    """x fp32 [rows,E] row r *= keep[r], in place (esmk_op_scale_rows)."""
    _req_cuda(x, keep)
    assert x.dtype == keep.dtype == torch.float32 and x.dim() == 2 and keep.numel() == x.shape[0]
    N.check(N.lib.esmk_op_scale_rows(N.ptr(x), N.ptr(keep), x.shape[0], x.shape[1], N.cur_stream()))
    return x


def msa_embed(tokens, tok_emb, pos_emb, msa_pos=None, pad_idx=1, x=None, keep=None, col_fill=None, any_pad=None):
    """MSA Transformer embedding (esmk_op_msa_embed): tokens int64 [B,R,C], tok_emb fp32 [vocab,D], pos_emb fp32 [npos,D],
    msa_pos fp32 [>= R, D] or None -> x fp32 [B,R,C,D], keep fp32 [B,R,C], col_fill fp32 [B,C,R], any_pad int32 [1]."""
    _req_cuda(tokens, tok_emb, pos_emb, msa_pos)
    assert tokens.dtype == torch.int64 and tokens.dim() == 3 and tok_emb.dtype == pos_emb.dtype == torch.float32
    B, R, C = tokens.shape
    vocab, D = tok_emb.shape
    npos = pos_emb.shape[0]
    assert pos_emb.shape[1] == D
    assert msa_pos is None or (msa_pos.dtype == torch.float32 and msa_pos.shape[-1] == D and msa_pos.numel() >= R * D)
    dev = tokens.device
    x = _out(x, (B, R, C, D), torch.float32, dev)
    keep = _out(keep, (B, R, C), torch.float32, dev)
    col_fill = _out(col_fill, (B, C, R), torch.float32, dev)
    any_pad = _out(any_pad, (1,), torch.int32, dev)
    N.check(N.lib.esmk_op_msa_embed(N.ptr(tokens), N.ptr(tok_emb), N.ptr(pos_emb), N.ptr(msa_pos), N.ptr(x), N.ptr(keep),
                                    N.ptr(col_fill), N.ptr(any_pad), B, R, C, D, vocab, pad_idx, npos, N.cur_stream()))
    return x, keep, col_fill, any_pad


def sinus_table(freq, T, pos0, out=None):
    """fp32 [T, 2 half]: row t = sin | cos of fp32(pos0 + t) * freq[i] (esmk_op_sinus_table); freq fp32 [half]."""
    _req_cuda(freq)
    assert freq.dtype == torch.float32 and freq.dim() == 1
    half = freq.numel()
    out = _out(out, (T, 2 * half), torch.float32, freq.device)
    N.check(N.lib.esmk_op_sinus_table(N.ptr(freq), N.ptr(out), T, half, pos0, N.cur_stream()))
    return out


def rope_table(inv_freq, T, cos=None, sin=None):
    """(cos, sin) fp32 [T, half] of fp32(t) * inv_freq[i] (esmk_op_rope_table); inv_freq fp32 [half]."""
    _req_cuda(inv_freq)
    assert inv_freq.dtype == torch.float32 and inv_freq.dim() == 1
    half = inv_freq.numel()
    cos = _out(cos, (T, half), torch.float32, inv_freq.device)
    sin = _out(sin, (T, half), torch.float32, inv_freq.device)
    N.check(N.lib.esmk_op_rope_table(N.ptr(inv_freq), N.ptr(cos), N.ptr(sin), T, half, N.cur_stream()))
    return cos, sin


def gather_rows(x, sel, out=None):
    """fp32 [n,E] = x[clamp(sel, 0, N - 1)] (esmk_op_gather_rows); x fp32 [N,E], sel int32 [n] on the device."""
    _req_cuda(x, sel)
    assert x.dtype == torch.float32 and x.dim() == 2 and sel.dtype == torch.int32 and sel.dim() == 1
    Nr, E = x.shape
    n = sel.numel()
    out = _out(out, (n, E), torch.float32, x.device)
    N.check(N.lib.esmk_op_gather_rows(N.ptr(x), N.ptr(sel), N.ptr(out), Nr, E, n, N.cur_stream()))
    return out


def stream_edit_desc(layer, op, keep, gain, rows=None, token_set=0, src=None, src_ld=None, src_index=None, n_rows=None):
    """The ``esmk_stream_edit`` descriptor of one edit (include/esmk.h) over device tensors, which the caller keeps alive:
    ``rows`` int32 [n] or None (then ``token_set``, bit v = token v); ``src`` fp32 [E] (``src_ld`` 0) or [n_src, ld] (``src_ld``
    its row stride unless given); ``src_index`` int32 or None.  ``n_rows``: the length of the list when it is not the tensor's
    (an EMPTY list is a tensor of one element with ``n_rows`` 0: an empty tensor has no address, and a null ``rows_dev``
    means the token selector)."""
    _req_cuda(rows, src, src_index)
    assert rows is None or (rows.dtype == torch.int32 and rows.numel() > 0)
    assert src is None or src.dtype == torch.float32
    assert src_index is None or src_index.dtype == torch.int32
    if src is None:
        ld, n_src = 0, 0
    elif src.dim() == 1:
        ld, n_src = 0, 1
    else:
        ld, n_src = src.stride(0), src.shape[0]
    if n_rows is None:
        n_rows = 0 if rows is None else rows.numel()
    return N.EsmkStreamEdit(int(layer), int(op), float(keep), float(gain), N.ptr(rows), int(n_rows), int(token_set), N.ptr(src), ld if src_ld is None else int(src_ld), n_src, N.ptr(src_index))


def stream_edit(x, op, keep=1.0, gain=1.0, rows=None, tokens=None, token_set=0, src=None, src_ld=None, src_index=None, y=None,
                mean=None, rstd=None):
    """One edit of the residual stream as a single launch (``esmk_op_stream_edit``): x fp32 [N, E] IN PLACE.  ``rows`` int32 [n]
    lists the edited rows, or (None) every row whose token (``tokens`` int64 [N]) is in ``token_set``.  op ``N.EDIT_AXPBY``:
    x' = keep x + gain s (no src: keep x); ``N.EDIT_PROJECT``: x' = x - gain <x, s> / <s, s> s.  With ``y`` (operand dtype
    [>= N, ldy], its row stride taken from the tensor), ``mean`` and ``rstd`` fp32 [N] the edited rows' LayerNorm-fold state
    is written as ``esmk_op_rowstats`` would from x'."""
    _req_cuda(x, tokens, y, mean, rstd)
    assert x.dtype == torch.float32 and x.dim() == 2
    assert tokens is None or (tokens.dtype == torch.int64 and tokens.numel() == x.shape[0])
    assert y is None or (y.dtype in (torch.float16, torch.bfloat16) and y.dim() == 2 and y.shape[0] >= x.shape[0])
    n_rows = None
    if rows is not None and rows.numel() == 0:
        rows, n_rows = torch.zeros(1, dtype=torch.int32, device=x.device), 0
    if src_index is not None and src_index.numel() == 0:
        src_index = None
    desc = stream_edit_desc(0, op, keep, gain, rows, token_set, src, src_ld, src_index, n_rows)
    code = N.F16 if y is None else N.dtype_code(y.dtype)
    N.check(N.lib.esmk_op_stream_edit(N.ptr(x), N.ptr(tokens), x.shape[0], x.shape[1], ctypes.byref(desc), N.ptr(y),
                                      0 if y is None else y.stride(0), N.ptr(mean), N.ptr(rstd), code, N.cur_stream()))
    return x


def pair_head(q, k, lse, w, bias=None, n_sym=None, key_bias=None, tokens=None, pad_idx=1, prepend_bos=True, append_eos=True):
    """The linear pairwise head of csrc/pair_head.hip on stacked operands: q, k [L,B,H,T,D] (fp16 / bf16, D = 64 or 128, q in
    the LOG2 domain: ``to_log2_domain``), lse [L,B,H,T] the NATURAL-log row log-sum-exp (as ``attention`` returns it; converted
    here as fp32(lse * log2 e) in fp64), w fp32 [L*H, C_out] with the ``n_sym`` symmetric outputs first (default: all), bias fp32
    [C_out] or None, key_bias fp32 [B,T] (0 / -inf) and / or tokens int64 [B,T] marking <pad> -> fp32 [B,S,S,C_out]:
    ``sum_c w[c,o] (P_c[i,j] + P_c[j,i]) + bias[o]`` for o < n_sym, ``sum_c w[c,o] P_c[i,j] + bias[o]`` for the rest."""
    _req_cuda(q, k, lse, w, bias, key_bias, tokens)
    L, B, H, T, D = q.shape
    assert q.dtype == k.dtype and q.shape == k.shape and q.is_contiguous() and k.is_contiguous()
    assert w.dtype == torch.float32 and w.dim() == 2 and w.shape[0] == L * H and w.is_contiguous()
    C_out = w.shape[1]
    n_sym = C_out if n_sym is None else int(n_sym)
    assert bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (C_out,) and bias.is_contiguous())
    assert key_bias is None or (key_bias.dtype == torch.float32 and tuple(key_bias.shape) == (B, T) and key_bias.is_contiguous())
    assert tokens is None or (tokens.dtype == torch.int64 and tuple(tokens.shape) == (B, T) and tokens.is_contiguous())
    lse2 = (lse.double() * LOG2E).float().contiguous()
    assert lse2.numel() == L * B * H * T
    bos, eos = int(prepend_bos), int(append_eos)
    S = T - bos - eos
    n = ctypes.c_size_t()
    N.check(N.lib.esmk_op_pair_head_workspace_bytes(H, L, ctypes.byref(n)))
    workspace = torch.empty(max(n.value, 1), dtype=torch.uint8, device=q.device)
    out = torch.empty((B, max(S, 0), max(S, 0), C_out), dtype=torch.float32, device=q.device)
    N.check(N.lib.esmk_op_pair_head(N.ptr(q), N.ptr(k), N.ptr(lse2), N.ptr(key_bias), N.ptr(tokens), N.ptr(w), N.ptr(bias), n_sym,
                                    C_out - n_sym, N.ptr(out), N.ptr(workspace), workspace.numel(), B, H, T, L, D, int(pad_idx), bos,
                                    eos, N.dtype_code(q.dtype), N.cur_stream()))
    return out


def distogram_energy(pair_logits, target_bin, first=0, n_bins=None, min_sep=0, inv_temp=1.0):
    """``(energy fp64 [B], count int32 [B])``: lm-design's categorical cross-entropy (utils/loss.py:10-29) of the ``n_bins``
    logits ``pair_logits[b, i, j, first:first + n_bins]`` (fp32 [B, S, S, ld], possibly a last-axis view of a wider tensor)
    against ``target_bin`` uint8 [S, S]: the mean over ALL ordered pairs with target_bin < n_bins (255 = ignore) and
    |i - j| >= ``min_sep`` of -log(softmax(inv_temp * logits)[target_bin] + 1e-8), in fp64.  The order of addition does not
    depend on B; no counted pair: 0.0."""
    _req_cuda(target_bin)
    if not pair_logits.is_cuda:
        raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
    assert pair_logits.dtype == torch.float32 and pair_logits.dim() == 4
    B, S, S2, width = pair_logits.shape
    n_bins = width - int(first) if n_bins is None else int(n_bins)
    # a last-axis slice of a contiguous [B, S, S, ld] tensor: the kernel takes ld and the first column
    ld = pair_logits.stride(2)
    assert pair_logits.stride(3) == 1 and pair_logits.stride(1) == S * ld and pair_logits.stride(0) == S * S * ld
    assert S == S2 and target_bin.dtype == torch.uint8 and tuple(target_bin.shape) == (S, S) and target_bin.is_contiguous()
    energy = torch.empty((B,), dtype=torch.float64, device=pair_logits.device)
    count = torch.empty((B,), dtype=torch.int32, device=pair_logits.device)
    # the base of the row space: the view's first column is folded into ``first``
    off = pair_logits.storage_offset() % ld if ld else 0
    base = pair_logits.data_ptr() - off * 4
    N.check(N.lib.esmk_op_distogram_energy(ctypes.c_void_p(base), ld, off + int(first), n_bins, N.ptr(target_bin), B, S,
                                           int(min_sep), float(inv_temp), N.ptr(energy), N.ptr(count), N.cur_stream()))
    return energy, count


# ---- sparse-autoencoder features of the stream (include/esmk.h: esmk_op_sae_rows ... esmk_op_sae_decode) -------------------
def sae_cand():
    """The number of active features of a row up to which ``sae_topk`` selects in LDS (``kSaeCand`` of csrc/sae.hip)."""
    return int(N.lib.esmk_op_sae_cand())


def _image_rows_args(x, rows, out, n):
    """``(N, E, n, out)`` of ``sae_rows`` and ``align_rows``: the checks of x fp32 [N, E] and rows int32 [>= n] or None, and the
    fp16 image [>= n, ld >= 3 Ep], the caller's or allocated."""
    _req_cuda(x, rows, out)
    assert x.dtype == torch.float32 and x.dim() == 2
    assert rows is None or (rows.dtype == torch.int32 and rows.dim() == 1)
    Nr, E = x.shape
    n = (Nr if rows is None else rows.numel()) if n is None else int(n)
    assert rows is None or rows.numel() >= n
    if out is None:
        out = torch.empty((n, 3 * ((E + 63) // 64 * 64)), dtype=torch.float16, device=x.device)
    assert out.dtype == torch.float16 and out.dim() == 2 and out.shape[0] >= n
    return Nr, E, n, out


def sae_rows(x, rows=None, b_dec=None, input_scale=1.0, out=None, n=None):
    """The f16x3 activation image of SAE inputs (``esmk_op_sae_rows``): x fp32 [N, E], rows int32 [n] or None (the first ``n``
    rows, default all) -> fp16 [>= n, ld >= 3 Ep] rows ``hi | hi | lo`` per 64-column K tile of u = input_scale * x - b_dec
    (Ep = E rounded up to 64, pad columns zero); ``out`` is the caller's (row stride taken from the tensor) or allocated."""
    Nr, E, n, out = _image_rows_args(x, rows, out, n)
    _req_cuda(b_dec)
    assert b_dec is None or (b_dec.dtype == torch.float32 and b_dec.numel() == E)
    N.check(N.lib.esmk_op_sae_rows(N.ptr(x), E, Nr, N.ptr(rows if n else None), n, N.ptr(b_dec), float(input_scale), N.ptr(out),
                                   out.shape[1], E, N.cur_stream()))
    return out


def sae_topk(z, k, threshold=0.0, k_sae=0, n=None, indices=None, values=None, n_active=None, want_cutoff=False, want_path=False,
             F=None):
    """Row-wise top-k of SAE pre-activations (``esmk_op_sae_topk``): z fp32 [>= n, ldz] of which the first ``F`` columns
    (default all) are features; ``threshold`` a float or fp32 [F] -> dict(indices int32 [n, k], values fp32 [n, k], n_active
    int32 [n]) and, when asked for, cutoff (uint64 keys as int64 [n]) and path int32 [n] (0: the LDS path, > 0: the radix
    select).  Output tensors may be the caller's ([>= n, k] / [>= n], written in place)."""
    _req_cuda(z, indices, values, n_active)
    assert z.dtype == torch.float32 and z.dim() == 2
    n = z.shape[0] if n is None else int(n)
    F = z.shape[1] if F is None else int(F)
    assert z.shape[0] >= n
    thr_t, thr_s = (threshold, 0.0) if isinstance(threshold, torch.Tensor) else (None, float(threshold))
    if thr_t is not None:
        _req_cuda(thr_t)
        assert thr_t.dtype == torch.float32 and thr_t.numel() == F
    dev = z.device
    indices = torch.empty((n, k), dtype=torch.int32, device=dev) if indices is None else indices
    values = torch.empty((n, k), dtype=torch.float32, device=dev) if values is None else values
    n_active = torch.empty((n,), dtype=torch.int32, device=dev) if n_active is None else n_active
    assert indices.dtype == torch.int32 and values.dtype == torch.float32 and n_active.dtype == torch.int32
    assert indices.shape[0] >= n and values.shape[0] >= n and n_active.shape[0] >= n
    assert tuple(indices.shape[1:]) == (k,) and tuple(values.shape[1:]) == (k,)
    cutoff = torch.zeros((max(n, 1),), dtype=torch.int64, device=dev) if want_cutoff else None
    path = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev) if want_path else None
    N.check(N.lib.esmk_op_sae_topk(N.ptr(z), z.shape[1], N.ptr(thr_t), thr_s, n, F, int(k), int(k_sae), N.ptr(indices),
                                   N.ptr(values), N.ptr(n_active), N.ptr(cutoff), N.ptr(path), N.cur_stream()))
    out = dict(indices=indices, values=values, n_active=n_active)
    if want_cutoff:
        out["cutoff"] = cutoff[:n]
    if want_path:
        out["path"] = path[:n]
    return out


def sae_segment_max(z, rows, seg_start, protein_max, protein_argmax, threshold=0.0, cutoff=None, row0=0, n=None, F=None):
    """``esmk_op_sae_segment_max``: protein_max fp32 [B, F] / protein_argmax int32 [B, F] updated IN PLACE from the chunk z fp32
    [>= n, ldz] holding rows row0 .. row0 + n of a row list; rows int32 [n, 2] the chunk's (sequence, position) pairs, seg_start
    int32 [B + 1] the sequences' row ranges in the whole list; cutoff: ``sae_topk``'s, for a top-k autoencoder."""
    _req_cuda(z, rows, seg_start, protein_max, protein_argmax, cutoff)
    assert z.dtype == torch.float32 and z.dim() == 2
    n = z.shape[0] if n is None else int(n)
    B, Fm = protein_max.shape
    F = Fm if F is None else int(F)
    assert F == Fm and z.shape[1] >= F and z.shape[0] >= n
    assert protein_max.dtype == torch.float32 and protein_argmax.dtype == torch.int32 and tuple(protein_argmax.shape) == (B, F)
    assert rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == 2 and rows.shape[0] >= n
    assert seg_start.dtype == torch.int32 and seg_start.numel() == B + 1
    assert cutoff is None or (cutoff.dtype == torch.int64 and cutoff.numel() >= n)
    thr_t, thr_s = (threshold, 0.0) if isinstance(threshold, torch.Tensor) else (None, float(threshold))
    if thr_t is not None:
        _req_cuda(thr_t)
        assert thr_t.dtype == torch.float32 and thr_t.numel() == F
    N.check(N.lib.esmk_op_sae_segment_max(N.ptr(z), z.shape[1], N.ptr(thr_t), thr_s, N.ptr(cutoff), N.ptr(rows if n else seg_start),
                                          N.ptr(seg_start), int(row0), n, F, B, N.ptr(protein_max), N.ptr(protein_argmax),
                                          N.cur_stream()))
    return protein_max, protein_argmax


def sae_decode(indices, values, w_dec, b_dec=None, inv_scale=1.0, out=None):
    """``esmk_op_sae_decode``: fp32 [n, E] = inv_scale * (b_dec + sum_r values[:, r] * w_dec[indices[:, r]]), one rounded product
    and one rounded add per term in rank order; index -1 is skipped.  indices int32 [n, k], values fp32 [n, k], w_dec fp32 [F, E]."""
    _req_cuda(indices, values, w_dec, b_dec, out)
    assert indices.dtype == torch.int32 and values.dtype == torch.float32 and indices.dim() == 2 and indices.shape == values.shape
    assert w_dec.dtype == torch.float32 and w_dec.dim() == 2
    n, k = indices.shape
    F, E = w_dec.shape
    assert b_dec is None or (b_dec.dtype == torch.float32 and b_dec.numel() == E)
    out = _out(out, (n, E), torch.float32, w_dec.device)
    if n:
        N.check(N.lib.esmk_op_sae_decode(N.ptr(indices), N.ptr(values), n, k, N.ptr(w_dec), N.ptr(b_dec), float(inv_scale),
                                         N.ptr(out), E, F, N.cur_stream()))
    return out


# ---- embedding-based alignment (include/esmk.h: esmk_op_align_rows ... esmk_op_align_traceback) -----------------------------
def align_panel():
    """The columns one wavefront of the alignment DP covers at once (``kPanel`` of csrc/align.hip)."""
    return int(N.lib.esmk_op_align_panel())


def align_rows(x, rows=None, cosine=True, b_side=False, out=None, n=None):
    """One of the two f16x3 operand images of the similarity GEMM (``esmk_op_align_rows``): x fp32 [N, E], rows int32 [n] or
    None (the first ``n`` rows, default all; a negative index gives a zero row) -> fp16 [>= n, ld >= 3 Ep], ``hi | hi | lo`` per
    64-column K tile, with ``b_side`` ``hi | lo | hi``; cosine: the rows are scaled to unit length first."""
    Nr, E, n, out = _image_rows_args(x, rows, out, n)
    N.check(N.lib.esmk_op_align_rows(N.ptr(x), E, Nr, N.ptr(rows if n else None), n, int(bool(cosine)), int(bool(b_side)),
                                     N.ptr(out), out.shape[1], E, N.cur_stream()))
    return out


def _align_s(S, table, n_rows, n_cols):
    _req_cuda(S, table)
    assert S.dtype == torch.float32 and S.dim() == 2
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 5
    n_rows = S.shape[0] if n_rows is None else int(n_rows)
    n_cols = S.shape[1] // 8 * 8 if n_cols is None else int(n_cols)
    assert n_rows <= S.shape[0] and n_cols <= S.shape[1]
    return n_rows, n_cols


def align_enhance(S, table, max_lb, n_rows=None, n_cols=None, ws=None):
    """``esmk_op_align_enhance``: the pair blocks of S fp32 [n_rows, ldS] that ``table`` (int64 [P, 5]) lists are replaced IN
    PLACE by the mean of their row and column z-scores.  ``ws``: fp32 scratch of at least 2 max_lb floats, or allocated."""
    n_rows, n_cols = _align_s(S, table, n_rows, n_cols)
    P = table.shape[0]
    if ws is None:
        ws = torch.empty((max(min(P, 1024), 1) * 2 * int(max_lb),), dtype=torch.float32, device=S.device)
    _req_cuda(ws)
    assert ws.dtype == torch.float32
    N.check(N.lib.esmk_op_align_enhance(N.ptr(S), S.shape[1], n_rows, n_cols, N.ptr(table), P, int(max_lb), N.ptr(ws), ws.numel(),
                                        N.cur_stream()))
    return S


def align_dp(S, table, mode, gap_open, gap_extend, max_la, max_lb, want_traceback=True, tb=None, n_rows=None, n_cols=None, ws=None,
             score=None, end=None, free_ends=0):
    """``esmk_op_align_dp_ex``: per listed pair the affine-gap DP on its block of S -> dict(score fp32 [P], end int32 [P, 2]) and, with
    ``want_traceback``, ``tb`` uint8 (the caller's, or allocated to hold what the table's offsets address — the table is then
    read on the host).  mode 0 global, 1 local.  ``ws``: the boundary-column scratch a side b beyond ``align_panel()`` needs.
    ``free_ends``: the free-end mask of global mode (1 a_start, 2 a_end, 4 b_start, 8 b_end; 0: plain global)."""
    n_rows, n_cols = _align_s(S, table, n_rows, n_cols)
    P = table.shape[0]
    dev = S.device
    score = _out(score, (P,), torch.float32, dev)
    end = _out(end, (P, 2), torch.int32, dev)
    if want_traceback and tb is None:
        t = table.cpu()
        need = int((t[:, 4] + t[:, 1] * ((t[:, 3] + 15) // 16 * 16)).max()) if P else 0
        tb = torch.zeros((max(need, 16),), dtype=torch.uint8, device=dev)
    if int(max_lb) > align_panel() and ws is None:
        ws = torch.empty((max(min(P, 16384), 1) * 2 * (int(max_la) + 1),), dtype=torch.float32, device=dev)
    _req_cuda(tb, ws)
    N.check(N.lib.esmk_op_align_dp_ex(N.ptr(S), S.shape[1], n_rows, n_cols, N.ptr(table), P, int(mode), int(free_ends),
                                      float(gap_open), float(gap_extend), int(max_la), int(max_lb), N.ptr(score), N.ptr(end),
                                      N.ptr(tb if want_traceback else None), tb.numel() if want_traceback else 0,
                                      int(bool(want_traceback)), N.ptr(ws), 0 if ws is None else ws.numel(), N.cur_stream()))
    out = dict(score=score, end=end)
    if want_traceback:
        out["tb"] = tb
    return out


def align_traceback(table, mode, end, tb, slot, cols, n_cols=None, n_match=None, start=None, free_ends=0, S_mask=None,
                    n_rows_S=None, n_cols_S=None):
    """``esmk_op_align_traceback_ex``: walks the bytes of ``align_dp`` from ``end`` -> dict(n_cols, n_match int32 [P], start int32
    [P, 2]); the columns go into the back of each pair's slot (first column ``slot[p]``, La + Lb long) of ``cols`` int32 [cap, 2].
    ``free_ends``: the mask ``align_dp`` ran with.  ``S_mask``: the S of ``align_dp`` — every match cell of every walked path is
    set to -inf in it, so that the next ``align_dp`` on it finds each pair's next path; pair blocks must not overlap."""
    _req_cuda(table, end, tb, slot, cols)
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 5
    assert end.dtype == torch.int32 and tb.dtype == torch.uint8 and slot.dtype == torch.int64 and cols.dtype == torch.int32
    P = table.shape[0]
    assert end.numel() == 2 * P and slot.numel() == P and cols.dim() == 2 and cols.shape[1] == 2
    dev = table.device
    n_cols = _out(n_cols, (P,), torch.int32, dev)
    n_match = _out(n_match, (P,), torch.int32, dev)
    start = _out(start, (P, 2), torch.int32, dev)
    ldS = rows_S = cols_S = 0
    if S_mask is not None:
        rows_S, cols_S = _align_s(S_mask, table, n_rows_S, n_cols_S)
        ldS = S_mask.shape[1]
    N.check(N.lib.esmk_op_align_traceback_ex(N.ptr(table), P, int(mode), int(free_ends), N.ptr(end), N.ptr(tb), tb.numel(),
                                             N.ptr(slot), N.ptr(cols), cols.shape[0], N.ptr(n_cols), N.ptr(n_match), N.ptr(start),
                                             N.ptr(S_mask), ldS, rows_S, cols_S, N.cur_stream()))
    return dict(n_cols=n_cols, n_match=n_match, start=start)


# ---- protein search on pooled embeddings (include/esmk.h: esmk_op_pool_rows, esmk_op_topk_merge) ----------------------------
def pool_rows(x, rows, seg_off, out=None):
    """The mean of listed rows per segment (``esmk_op_pool_rows``): x fp32 [N, ldx >= E], rows int32 [n] or None (row r is list
    entry r), seg_off int32 [n_seg + 1] the segments' ranges in the list -> fp32 [n_seg, E]; the sum in fp64 in list order, an
    empty segment gives a zero row.  ``out``'s width is E (default: x's)."""
    _req_cuda(rows, seg_off, out)
    if not x.is_cuda:
        raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1  # (rows may be wider than E: ldx is the row stride)
    assert rows is None or (rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous())
    assert seg_off.dtype == torch.int32 and seg_off.dim() == 1 and seg_off.numel() >= 1 and seg_off.is_contiguous()
    n_seg = seg_off.numel() - 1
    if out is None:
        out = torch.empty((n_seg, x.shape[1]), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n_seg
    N.check(N.lib.esmk_op_pool_rows(N.ptr(x), x.stride(0), x.shape[0], N.ptr(rows), N.ptr(seg_off), n_seg, N.ptr(out), out.shape[1],
                                    N.cur_stream()))
    return out


def topk_merge(S, k, values=None, ids=None, n_cols=None, id_base=0, exclude=None, first=True, n_rows=None):
    """One block of a streaming row-wise top-k (``esmk_op_topk_merge``): S fp32 [n_rows, ldS] of which the first ``n_cols``
    columns are candidates (value, id_base + column); NaN values and the column whose id is ``exclude[row]`` (int32 [n_rows]) are
    none.  Unless ``first``, the used slots of the running lists ``values`` fp32 / ``ids`` int32 [n_rows, k] are candidates too.
    The lists receive the k best, value descending (IEEE total order), then id ascending; unused slots hold (-inf, -1)."""
    _req_cuda(values, ids, exclude)
    if not S.is_cuda:
        raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
    assert S.dtype == torch.float32 and S.dim() == 2 and S.stride(1) == 1  # (a view of wider rows: ldS is the row stride)
    n_rows = S.shape[0] if n_rows is None else int(n_rows)
    n_cols = S.shape[1] if n_cols is None else int(n_cols)
    assert n_rows <= S.shape[0] and n_cols <= S.shape[1]
    if values is None:
        assert first, "topk_merge: a running list is needed unless first"
        values = torch.empty((n_rows, int(k)), dtype=torch.float32, device=S.device)
        ids = torch.empty((n_rows, int(k)), dtype=torch.int32, device=S.device)
    assert values.dtype == torch.float32 and ids.dtype == torch.int32 and values.is_contiguous() and ids.is_contiguous()
    assert tuple(values.shape) == (n_rows, int(k)) and tuple(ids.shape) == (n_rows, int(k))
    assert exclude is None or (exclude.dtype == torch.int32 and exclude.is_contiguous() and exclude.numel() >= n_rows)
    N.check(N.lib.esmk_op_topk_merge(N.ptr(S), S.stride(0), n_rows, n_cols, int(id_base), N.ptr(exclude), int(k), N.ptr(values),
                                     N.ptr(ids), int(bool(first)), N.cur_stream()))
    return values, ids


# ---- range search and greedy clustering (include/esmk.h: esmk_op_range_rows, esmk_op_cluster_mark / _decide / _assign) ------
def range_rows(S, threshold, counts=None, offsets=None, cursor=None, ids=None, scores=None, n_cols=None, id_base=0, exclude=None,
               n_rows=None):
    """One block of a thresholded row scan (``esmk_op_range_rows``): S fp32 [n_rows, ldS]; column j < ``n_cols`` of row q passes
    when ``S[q][j] >= threshold`` (a float comparison) and ``id_base + j != exclude[q]``.  With ``counts`` (int64 [n_rows]) the
    count pass: the passing columns of every row are added to it.  With ``offsets`` (int64 [n_rows + 1]), ``cursor`` (int64
    [n_rows]), ``ids`` (int32 [cap]) and ``scores`` (fp32 [cap]) the fill pass: row q's passing (id, score) pairs go, in
    ascending column order, behind ``cursor[q]``, which advances; nothing is written at or behind ``offsets[q + 1]``."""
    _req_cuda(counts, offsets, cursor, ids, scores, exclude)
    if not S.is_cuda:
        raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
    assert S.dtype == torch.float32 and S.dim() == 2 and S.stride(1) == 1  # (a view of wider rows: ldS is the row stride)
    n_rows = S.shape[0] if n_rows is None else int(n_rows)
    n_cols = S.shape[1] if n_cols is None else int(n_cols)
    assert n_rows <= S.shape[0] and n_cols <= S.shape[1]
    fill = counts is None
    if fill:
        assert offsets is not None and cursor is not None and ids is not None and scores is not None, "range_rows: counts, or the four fill arrays"
        assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.numel() >= n_rows + 1
        assert cursor.dtype == torch.int64 and cursor.is_contiguous() and cursor.numel() >= n_rows
        assert ids.dtype == torch.int32 and scores.dtype == torch.float32 and ids.is_contiguous() and scores.is_contiguous()
        assert ids.dim() == 1 and ids.numel() == scores.numel()
    else:
        assert offsets is None and cursor is None and ids is None and scores is None, "range_rows: counts, or the four fill arrays"
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= n_rows
    assert exclude is None or (exclude.dtype == torch.int32 and exclude.is_contiguous() and exclude.numel() >= n_rows)
    N.check(N.lib.esmk_op_range_rows(N.ptr(S), S.stride(0), n_rows, n_cols, int(id_base), N.ptr(exclude), float(threshold), int(fill),
                                     N.ptr(counts), N.ptr(offsets), N.ptr(cursor), N.ptr(ids), N.ptr(scores),
                                     ids.numel() if fill else 0, N.cur_stream()))
    return cursor if fill else counts


def _req_graph(offsets, ids, rank, state):
    _req_cuda(offsets, ids, rank, state)
    n = rank.numel()
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.numel() == n + 1
    assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.dim() == 1
    assert rank.dtype == torch.int32 and rank.is_contiguous() and state.dtype == torch.int32 and state.is_contiguous() and state.numel() == n
    return n


def cluster_mark(offsets, ids, rank, state, blocked, covered, lanes=64):
    """The mark launch of a clustering round (``esmk_op_cluster_mark``) on the CSR ``offsets`` int64 [n + 1] / ``ids`` int32
    [nnz]: an undecided u (state 0) sets ``blocked[w]``, a new representative u (state 1) sets ``covered[w]``, for every w of
    its out-list with ``rank[w] > rank[u]``.  ``lanes`` consecutive lanes walk one out-list."""
    n = _req_graph(offsets, ids, rank, state)
    _req_cuda(blocked, covered)
    for t in (blocked, covered):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
    N.check(N.lib.esmk_op_cluster_mark(N.ptr(offsets), N.ptr(ids), n, ids.numel(), N.ptr(rank), N.ptr(state), N.ptr(blocked),
                                       N.ptr(covered), int(lanes), N.cur_stream()))


def cluster_decide(state, blocked, covered, remaining):
    """The decide launch of a clustering round (``esmk_op_cluster_decide``): state 1 -> 2; an undecided node becomes covered (3)
    if ``covered`` is set, a new representative (1) unless ``blocked`` is; ``blocked`` is cleared; the nodes left undecided are
    added to ``remaining`` (int32 [1])."""
    _req_cuda(state, blocked, covered, remaining)
    n = state.numel()
    for t in (state, blocked, covered):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
    assert remaining.dtype == torch.int32 and remaining.numel() >= 1
    N.check(N.lib.esmk_op_cluster_decide(N.ptr(state), N.ptr(blocked), N.ptr(covered), n, N.ptr(remaining), N.cur_stream()))


def cluster_assign(offsets, ids, scores, rank, state, nearest, key=None, lanes=64):
    """The assignment (``esmk_op_cluster_assign``): key int64 [n] (the bits of a uint64; zeroed here unless given) receives per
    node the maximum of ``[order(score) or 0] << 32 | 0xFFFFFFFF - rank[u]`` over the representatives u that list it and
    rank before it.  0 stays where no representative does."""
    n = _req_graph(offsets, ids, rank, state)
    _req_cuda(scores, key)
    assert scores is None or (scores.dtype == torch.float32 and scores.is_contiguous() and scores.numel() == ids.numel())
    if key is None:
        key = torch.zeros((n,), dtype=torch.int64, device=rank.device)
    assert key.dtype == torch.int64 and key.is_contiguous() and key.numel() == n
    N.check(N.lib.esmk_op_cluster_assign(N.ptr(offsets), N.ptr(ids), N.ptr(scores), n, ids.numel(), N.ptr(rank), N.ptr(state),
                                         int(bool(nearest)), N.ptr(key), int(lanes), N.cur_stream()))
    return key


# ---- search hits to an MSA (include/esmk.h: esmk_op_msa_project, esmk_op_msa_pair_identity) ---------------------------------
def msa_project(cols, col_offsets, seqs, seq_off, seq_len, query, ld=None, msa=None, stats=None):
    """The alignment paths of the P hits of one query as rows of a byte matrix (``esmk_op_msa_project``): (msa uint8 [P, ld],
    stats int32 [P, 6]).  ``cols`` int32 [n, 2] and ``col_offsets`` int64 [P + 1] as ``align`` returns them — the offsets index
    into ``cols``, so the hits of one query are given by their slice of the offsets and the whole of ``cols``; ``seqs`` uint8
    [n_bytes], hit p's residues at ``seq_off[p]`` (int64 [P]), ``seq_len[p]`` (int32 [P]) of them; ``query`` uint8 [Lq].
    Row p is '-' in the columns below Lq except ``msa[p][i] = seqs[seq_off[p] + j]`` for every match (i, j) of its path, and 0
    from Lq to ``ld`` (default: Lq rounded up to 4).  stats: n_match, n_ident, n_ins, n_del, first and last matched query column."""
    _req_cuda(cols, col_offsets, seqs, seq_off, seq_len, query, msa, stats)
    assert cols.dtype == torch.int32 and cols.dim() == 2 and cols.shape[1] == 2
    assert col_offsets.dtype == torch.int64 and col_offsets.dim() == 1 and col_offsets.numel() >= 1
    P = col_offsets.numel() - 1
    assert seqs.dtype == torch.uint8 and seqs.dim() == 1 and query.dtype == torch.uint8 and query.dim() == 1
    assert seq_off.dtype == torch.int64 and seq_off.numel() == P and seq_len.dtype == torch.int32 and seq_len.numel() == P
    Lq = query.numel()
    ld = (Lq + 3) // 4 * 4 if ld is None else int(ld)
    dev = query.device
    if msa is None:
        msa = torch.empty((P, ld), dtype=torch.uint8, device=dev)
    if stats is None:
        stats = torch.empty((P, 6), dtype=torch.int32, device=dev)
    assert msa.dtype == torch.uint8 and msa.dim() == 2 and msa.shape[0] >= P and msa.shape[1] == ld
    assert stats.dtype == torch.int32 and stats.numel() >= 6 * P
    if P == 0:  # (empty tensors have no address to hand over)
        return msa, stats
    N.check(N.lib.esmk_op_msa_project(N.ptr(cols), cols.shape[0], N.ptr(col_offsets), P, N.ptr(seqs), seqs.numel(), N.ptr(seq_off),
                                      N.ptr(seq_len), N.ptr(query), Lq, N.ptr(msa), ld, N.ptr(stats), N.cur_stream()))
    return msa, stats


def msa_pair_identity(msa, L=None, gap=ord("-"), min_overlap=1, i0=0, nb=None, out=None):
    """Rows ``i0 .. i0 + nb - 1`` (default: all) of the gap-aware pairwise identity of ``msa`` uint8 [N, ld] over its first ``L``
    columns (``esmk_op_msa_pair_identity``): fp32 [nb, N rounded up to 4], ``S[r][j] = same / both`` — ``both`` the columns
    in which neither row holds the byte ``gap``, ``same`` those in which the two bytes are equal — where ``both >= min_overlap``
    and 0 elsewhere; the columns behind N are 0.  A block is what ``range_rows`` takes (``n_cols=N``).  ``msa`` may be a view
    with a row stride (odd strides and bases take the byte-wise loads)."""
    if not msa.is_cuda:
        raise RuntimeError("esm_amd.ops: tensors must live on the GPU (no CPU fallback)")
    assert msa.dtype == torch.uint8 and msa.dim() == 2 and (msa.shape[1] == 1 or msa.stride(1) == 1)
    N_, ld = msa.shape[0], (msa.stride(0) if msa.shape[0] > 1 else msa.shape[1])
    L = msa.shape[1] if L is None else int(L)
    if N_ < 1 or not 1 <= L <= msa.shape[1]:
        raise ValueError(f"msa: need at least one row and 1 <= L <= {msa.shape[1]} columns, got N = {N_}, L = {L}")
    nb = N_ - int(i0) if nb is None else int(nb)
    ldS = (N_ + 3) // 4 * 4
    if out is None:
        out = torch.empty((max(nb, 0), ldS), dtype=torch.float32, device=msa.device)
    _req_cuda(out)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] >= nb and out.shape[1] == ldS
    N.check(N.lib.esmk_op_msa_pair_identity(N.ptr(msa), N_, L, ld, int(gap), int(min_overlap), int(i0), nb, N.ptr(out), ldS,
                                            N.cur_stream()))
    return out
