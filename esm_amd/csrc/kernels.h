// kernels.h — host-side declarations of the kernel launchers (internal to libesmk.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace esmk {

enum { ESMK_DT_F32 = 0, ESMK_DT_F16 = 1, ESMK_DT_BF16 = 2 };

enum {
    EPI_STORE_T = 0,    // out[M,N] operand dtype = acc + bias
    EPI_STORE_F32 = 1,  // out[M,N] fp32          = acc + bias
    EPI_GELU_T = 2,     // out operand dtype      = gelu(acc + bias)
    EPI_GELU_F32 = 3,   // out fp32               = gelu(acc + bias)
    EPI_RESID_F32 = 4,  // out fp32              += acc + bias
    EPI_QKV_ROPE = 5,   // fused q,k projection: bias, q scale, RoPE, head-major store (head_dim 64)
    EPI_V_T = 6,        // v projection stored transposed [B,H,64,Tp] for the attention kernel
    EPI_MSA_CTX = 7,    // MSA row attention context: out[((zo*R + n/64)*C + m)*ldc + zi*64 + n%64] (operand dtype)
    // q, k and v in ONE launch (gemm9 only, half-height tiles, plain or LayerNorm-fold consumer form; N = 3E, W and bias = the packed [3E] q | k | v rows, E a multiple of 128): tiles
    // of columns [0,2E) run exactly as EPI_QKV_ROPE, tiles of [2E,3E) exactly as EPI_V_T — the same instruction sequence per
    // tile as the two launches, hence the same bits; what changes is how many ROUNDS of tiles the 256 CUs need (small batches)
    EPI_QKV_ALL = 8
};

struct GemmArgs {
    const void* A = nullptr;      // [M,K] operand dtype
    const void* W = nullptr;      // [N,K] operand dtype
    const float* bias = nullptr;  // [N] or null
    void* out = nullptr;
    int M = 0, N = 0, K = 0;
    int force_generic = 0;
    int force_old = 0;  // use the one-tile-per-workgroup kernels of gemm.hip (A/B measurements, tests)
    int panel_c = 0;    // gemm8: N tiles per column panel of the tile order (0 = choose)
    int half_m = 0;     // gemm8: 128-row tiles: 0 = decide from the tile count, 1 = force, -1 = never (A/B, tests)
    int xpf_kt = -1;    // gemm8, EPI_RESID_F32: K tile after which the residual tile is prefetched into the L2 (set by the launcher)
    // EPI_QKV_ROPE only
    void* q = nullptr;   // [B,H,T,64]
    void* k = nullptr;   // [B,H,T,64]
    void* vt = nullptr;  // [B,H,64,Tp]
    const float* cos = nullptr;  // [T,32]
    const float* sin = nullptr;  // [T,32]
    int T = 0, H = 0, E = 0, Tp = 0;
    float scaling = 1.f;
    // ---- generalised addressing of the persistent kernel (gemm8.hip); 0 = dense default ------------
    long long a_row_bytes = 0, w_row_bytes = 0;  // stride between consecutive operand rows (2K)
    long long a_kt_bytes = 0, w_kt_bytes = 0;    // stride between consecutive 64-wide K tiles (128)
    int a_kt_repeat = 0;                         // 1: the A stream stays on each K tile for TWO stream positions (split
                                                 // weights, W = W_hi + W_lo stored as interleaved K tiles [hi0 lo0 hi1 ...]:
                                                 // K counts the 2 K_real columns of that image, a_row_bytes = 2 K_real)
    int batch = 1, batch_inner = 1;              // batched GEMM: z = zo * batch_inner + zi
    long long a_bo = 0, a_bi = 0, w_bo = 0, w_bi = 0, o_bo = 0, o_bi = 0;  // byte offsets per zo / zi
    int n_valid = 0;                  // W rows that exist (default N): loads of rows >= n_valid are clamped
    int ldc = 0;                      // output row stride in elements (default N)
    const float* row_keep = nullptr;  // EPI_QKV_ROPE: q row m is multiplied by row_keep[m] (axial_attention.py:85-88)
    int vt_rows = 0;                  // EPI_V_T: > 0 selects the layout [B,H,R = vt_rows,64,Tp], keys not permuted
    int rowmap_R = 0, rowmap_C = 0;   // EPI_RESID_F32: GEMM row (b,c,r) is added to output row (b,r,c)
    int ctx_R = 0, ctx_C = 0;         // EPI_MSA_CTX geometry
    int head_dim = 64;                // EPI_QKV_ROPE / EPI_V_T: 64, or 128 (two 64-column slices per head)
    const int* row_pos = nullptr;     // EPI_QKV_ROPE: rotary position of row m (token-packed batches; default m % T)
    // ---- LayerNorm fold (gemm9 only) ------------------------------------------------------------
    // Producer = EPI_RESID_F32 with ln_part != null: besides out[m][n] += acc + bias it writes the operand-dtype copy
    // h16[m][n] = T(out_new - ln_mean[m]) (row stride ldh) that the next GEMM takes as its A operand, and the partial
    // row sums ln_part[(m * ln_parts + n_base / 128) * 2 + {0, 1}] = (sum d, sum d^2) over the wave's 128 columns,
    // d = out_new - ln_mean[m] (ln_mean: the row's PREVIOUS mean — any per-row constant cancels against the centred
    // weights; it only keeps the rounding of h16 relative to the row's spread instead of its offset).
    // Consumer = EPI_QKV_ROPE / EPI_V_T / EPI_GELU_T with ln_rstd != null: W holds gamma-folded, row-centred weights,
    // the accumulators start from 0 and the epilogue computes  ln_rstd[m] * acc + (bias[n] + bias2[n])
    // (bias2 = W . beta, written when the weights were folded).
    void* h16 = nullptr;
    int ldh = 0;
    float* ln_part = nullptr;
    int ln_parts = 0;
    const float* ln_mean = nullptr;
    const float* ln_rstd = nullptr;
    const float* bias2 = nullptr;
    // Precision mode f16x3, EPI_GELU_T: the output rows leave as the A operand of that mode's fc2 — per 64-column K tile
    // hi | hi | lo, lo = T(v - T(v)), row stride 3 N; full-height gemm9 instantiation of its own
    int x3_out = 0;
};

// gemm_dispatch.hip: the kernel choice.  gemm_plan is the pure decision (no HIP call), launch_gemm = gemm_plan + one
// switch over plan.kernel
struct GemmPlan {
    int kernel = 0;   // 9 (gemm9.hip), 8 (gemm8.hip), 256 / 64 (the tile kernels of gemm.hip), 0 = no kernel takes this call
    int half_m = 0;   // 1: 128-row tiles (the persistent kernels)
};
GemmPlan gemm_plan(const GemmArgs& p, int epi);
hipError_t launch_gemm(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st);
bool gemm_qkv_one_launch(const GemmArgs& qk);  // q / k and v as one EPI_QKV_ALL launch: supported and fewer rounds of tiles?
// which persistent kernel serves dense calls: 8, 9 or 0 = by rule (ESMK_GEMM_IMPL / esmk_debug_gemm_impl); false: var != 0
// (gemm9 once had variants; the C ABI keeps the argument)
bool gemm_set_impl(int impl, int var);
// switches by name (esmk_debug_set): "qkv_one_launch".  false: unknown key
bool gemm_set_knob(const char* key, double value);
// gemm.hip: one tile per workgroup — 256 x 256 (K % 64 == 0, N % 8 == 0) and the generic 64 x 64 (K % 32 == 0); dense calls
int gemm_tile_kernel(const GemmArgs& p, int epi);  // 256, 64 or 0 = neither takes the call
hipError_t launch_gemm256(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st);
hipError_t launch_gemm64(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st);
// gemm8.hip: persistent ping-pong kernel (K % 64 == 0, N % 8 == 0), dense and generalised addressing
bool gemm8_supports(const GemmArgs& p, int epi);
bool gemm8_generalised(const GemmArgs& p, int epi);  // uses fields only the persistent kernel implements
bool gemm8_half_height(const GemmArgs& p);            // dense kernels: 128 x 256 tiles for this shape?
hipError_t launch_gemm8(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st);
// gemm32.hip: fp32 in / fp32 accumulate / fp32 out on the exact-fp32 MFMA path (1/16 of the fp16 rate): the LM head of
// the f16x2 precision mode.  A [M,K] row stride lda, W [N,K], out [M,N] row stride ldc; K % 32 == 0, lda % 4 == 0
hipError_t launch_gemm32(const float* A, int lda, const float* W, const float* bias, float* out, int ldc, int M, int N,
                         int K, bool gelu, hipStream_t st);
// measurement hook: per-tile s_memtime stamps of workgroup-leader lanes ([workgroup][tile & 31][4])
void gemm8_set_timing(unsigned long long* dev_buf);
// gemm9.hip: the same contract on one wave per SIMD (128 x 128 wave blocks); dense operands only
bool gemm9_supports(const GemmArgs& p, int epi);
bool gemm9_ln_fold(const GemmArgs& p, int epi);  // the call asks for the LayerNorm-fold form of its epilogue
hipError_t launch_gemm9(const GemmArgs& p, int epi, int operand_dtype, hipStream_t st);
void gemm9_set_timing(unsigned long long* dev_buf);

// ---- elementwise.hip -------------------------------------------------------------------
// per-sequence statistics of the token matrix (esm2.py:82,86-92): scale[b] for token dropout,
// key_bias[b,t] = 0 / -inf (multihead_attention.py:368-374), seq_info[2b] = #pads (esm2.py:108-109),
// seq_info[2b+1] = 1 + index of the last non-pad token
hipError_t launch_seq_stats(const int64_t* tokens, int B, int T, int pad_idx, int mask_idx,
                            int token_dropout, float* scale, float* key_bias, int* seq_info,
                            hipStream_t st, float* keep = nullptr);  // keep[b,t] = 1 - pad (optional)
// ESM-1b / ESM-1v: x += embed_positions[...] (esm1.py:133, modules.py:240-257); x *= keep (esm1.py:138-139)
// seg != null: token-packed batch, "sequence" b = segment b = rows [seg[2b], seg[2b] + seg[2b+1]), T = longest
hipError_t launch_add_positions(const int64_t* tokens, const float* pos_emb, float* x, int B, int T, int E,
                                int pad_idx, int npos, hipStream_t st, const int* seg = nullptr);
hipError_t launch_scale_rows(float* x, const float* keep, int rows, int E, hipStream_t st);
// embedding gather + token-dropout rescale + pad zeroing (esm2.py:84-95)
hipError_t launch_embed(const int64_t* tokens, const float* table, const float* scale, float* x,
                        int B, int T, int E, int vocab, int pad_idx, int mask_idx,
                        int token_dropout, hipStream_t st);
// ESM-1 embedding (esm1.py:123-133): x = embed_scale * embed[tok], token dropout as above, + sinus[t] on non-pad tokens
// (SinusoidalPositionalEmbedding, modules.py:260-295: position pad_idx + 1 + t, pads take the zero row); no pad zeroing
hipError_t launch_embed_esm1(const int64_t* tokens, const float* table, const float* scale, const float* sinus, float* x,
                             int B, int T, int E, int vocab, int pad_idx, int mask_idx, int token_dropout,
                             float embed_scale, hipStream_t st);
// sinus[t][0 .. half) = sin((pos0 + t) freq[i]), [half .. 2 half) = cos(...), fp32, precise sinf / cosf; row stride 2 half
hipError_t launch_sinus_table(const float* freq, float* table, int T, int half, int pos0, hipStream_t st);
// LayerNorm(E, eps=1e-5) (modules.py:68-81): fp32 rows -> operand-dtype and/or fp32 rows
hipError_t launch_layernorm(const float* x, const float* gamma, const float* beta, void* y,
                            float* y32, int rows, int E, int operand_dtype, hipStream_t st);
// LayerNorm fold (elementwise.hip): entry of the chain, statistics from the producers' partial sums,
// load-time weight fold
hipError_t launch_rowstats(const float* x, void* y, float* mean, float* rstd, int rows, int E, int ldy, int operand_dtype,
                           hipStream_t st);
hipError_t launch_ln_finalize(const float* part, float* mean, float* rstd, int rows, int parts, int E, hipStream_t st);
hipError_t launch_fold_weight(const void* src, int src_dtype, const float* gamma, const float* beta, void* dst, int dst_dtype,
                              float* bias2, size_t rows, size_t cols, size_t dst_ld, int row_map, int d, hipStream_t st);
// interventions.hip — one edit of the fp32 residual stream x [N, E] in place (include/esmk.h, esmk_op_stream_edit: the
// semantics).  rows != null: the listed rows (entries outside [0, N) are skipped), else every row whose token is in
// token_set.  y != null: the edited rows' fold-chain state (y = T(x' - mean), mean, rstd) by rowstats_kernel's arithmetic.
struct StreamEditArgs {
    float* x = nullptr;
    const int64_t* tokens = nullptr;  // [N]; read under the token selector only
    const int* rows = nullptr;
    int n_rows = 0;
    unsigned long long token_set = 0;
    const float* src = nullptr;  // row stride src_ld: 0 = one vector for every row, else >= E; n_src rows
    int src_ld = 0, n_src = 0;
    const int* src_index = nullptr;  // [n_rows] (token selector: [N]); null: source row i of listed row i / of row r
    float keep = 1.f, gain = 0.f;
    int op = 0;  // ESMK_EDIT_AXPBY | ESMK_EDIT_PROJECT
    void* y = nullptr;
    int ldy = 0;
    float *mean = nullptr, *rstd = nullptr;
    int N = 0, E = 0;
};
hipError_t launch_stream_edit(const StreamEditArgs& a, int operand_dtype, hipStream_t st);
// MSA Transformer variants of the same kernel: output rows scaled by row_keep[row] (padded positions
// zeroed, msa_transformer.py:171-172) and/or written in (b,c,r) row order for the column-attention block
struct LnExtra {
    const float* row_keep = nullptr;
    int map_R = 0, map_C = 0;
    int ldy = 0;  // row stride of the operand-dtype output in elements (0 = E): K-padded activation rows
    int x3 = 0;   // precision mode f16x3: y rows in the hi | hi | lo layout per 64-column K tile (ldy >= 3 E), lo = T(o - T(o))
    float eps = 1e-5f;  // 1e-12 for ESM-1 (ESM1LayerNorm, modules.py:44-65: the same formula)
};
hipError_t launch_layernorm_ex(const float* x, const float* gamma, const float* beta, void* y,
                               float* y32, int rows, int E, int operand_dtype, LnExtra ex,
                               hipStream_t st);
// MSA embedding (msa_transformer.py:152-165, modules.py:240-257) and padding bookkeeping
hipError_t launch_msa_embed(const int64_t* tokens, const float* tok_emb, const float* pos_emb,
                            const float* msa_pos, float* x, float* keep, float* col_fill, int* any_pad,
                            int B, int R, int C, int D, int vocab, int pad_idx, int npos, hipStream_t st);
// tied row attention softmax (axial_attention.py:96-100,127)
hipError_t launch_msa_row_softmax(const float* scores, const float* keep, const int* any_pad, void* probs,
                                  float* attn_out, int B, int H, int R, int C, int ldp, int layer,
                                  int num_layers_total, int operand_dtype, hipStream_t st, int nslice = 1);
// dtype conversion of a parameter tensor into the packed image
hipError_t launch_convert(const void* src, int src_dtype, void* dst, int dst_dtype, size_t n,
                          hipStream_t st);
// [rows, cols] -> dst with row stride dst_ld; row_map / col_map = 1 spreads head_dim-d heads over 64 slots
hipError_t launch_convert2d(const void* src, int src_dtype, void* dst, int dst_dtype, size_t rows, size_t cols,
                            size_t dst_ld, int row_map, int col_map, int d, hipStream_t st);
// split-weight image (operand mode f16x2): src [rows, cols] -> dst fp16 [rows, 2 dst_ld]; 64-column K tile t of row r
// becomes hi = fp16(w) at dst[r][128 t .. +63] and lo = fp16(w - hi) at dst[r][128 t + 64 .. +127]
// (hi + lo carries ~19-22 bits of w: the MFMA takes fp16 subnormals as they are); row_map / col_map as above
// parts = 3 (operand mode f16x3): hi | lo | hi per K tile, rows of 3 dst_ld — against activation rows hi | hi | lo
// (LnExtra::x3, GemmArgs::x3_out, attention's X3 output) a plain GEMM over K' = 3 K is A_hi W_hi + A_hi W_lo + A_lo W_hi
hipError_t launch_convert2d_split(const void* src, int src_dtype, void* dst, size_t rows, size_t cols, size_t dst_ld,
                                  int row_map, int col_map, int d, hipStream_t st, int parts = 2);
// the f16x3 image of n gathered fp32 activation rows: out fp16 [n, ldo >= 3 Ep], row i = hi | hi | lo (b_side: hi | lo | hi) per K
// tile of u = x[rows[i]] * s - b_dec (one rounding each), s = scale or, with cosine, float32(1 / sqrt(fp64 sum x^2)); rows
// int32 [n] or null (row i), clamped to [0,N), with zero_negative a negative index gives a zero row; b_dec fp32 [E] or null
hipError_t launch_image_rows(const float* x, int ldx, int N, const int* rows, int n, const float* b_dec, float scale, int cosine,
                             int b_side, int zero_negative, void* out, int ldo, int E, hipStream_t st);
// RoPE tables cos/sin[t][i] = cos/sin(t * inv_freq[i]) (rotary_embedding.py:47-61), fp32
hipError_t launch_rope_table(const float* inv_freq, float* cos, float* sin, int T, int half,
                             hipStream_t st);
hipError_t launch_copy_f32(const float* src, float* dst, size_t n, hipStream_t st);
// out[b,:] = mean of rows [first, first + min(count[b], T - first)) of x[b] ([B,T,E], any dtype code); NaN if empty
hipError_t launch_masked_row_mean(const void* x, int x_dtype, const int* count, float* out, int B, int T, int E,
                                  int first, hipStream_t st);
// scoring.hip — the token copies of variant scoring (esmk_forward_rows), windowed scoring and the categorical Jacobian, one
// kernel.  out int64 [n,Tw]: copy i, column c = tokens[src_row[i], start[i] + c - h] (h = 1 if head_tok >= 0; row and column
// clamped; src_row null: row 0, start null: 0), column 0 = head_tok and column Tw - 1 = tail_tok where those are >= 0; the
// entries of pos[pos_off[i] : pos_off[i+1]] (SOURCE token coordinates; pos_off int32 [n+1] clamped to [0,total], hi < lo: none;
// pos_off null: pos[i] alone) that land on a body column become mask_idx, or with tok (int32 [n]) tok[i], a tok[i] outside
// [0,V) substituting nothing.  esmk_op_mask_rows: pos; _mask_rows_multi: pos_off, pos; _substitute_rows: pos, tok (all three
// Tw = T, no head or tail); _window_rows: everything but tok
hipError_t launch_copy_rows(const int64_t* tokens, const int* src_row, const int* start, const int* pos_off, const int* pos,
                            const int* tok, int64_t* out, int B, int T, int n, int Tw, int total, int V, int head_tok, int tail_tok,
                            int mask_idx, hipStream_t st);
// mask_rows_multi into ONE packed row space of `rows` rows (esmk_forward_packed_rows): copy i = the first seg_len[i] tokens of
// tokens[src_row[i]] at out[seg_start[i] ...], its positions masked, the gap up to seg_start[i+1] (rows for the last copy) filled
// with pad_idx; src_row, seg_start, seg_len int32 [n] (clamped: row to [0,B), length to [0,T], written range to [0,rows))
hipError_t launch_mask_rows_packed(const int64_t* tokens, const int* src_row, const int* seg_start, const int* seg_len,
                                   const int* pos_off, const int* pos, int64_t* out, int B, int T, int n, int total, int rows,
                                   int mask_idx, int pad_idx, hipStream_t st);
// out [n,E] = rows sel[i] (clamped to [0,N)) of x [N,E], fp32, E % 4 == 0
hipError_t launch_gather_rows(const float* x, const int* sel, float* out, int N, int E, int n, hipStream_t st);
// out [n,V] = log_softmax(logits [n,V]), V <= 64; target (optional, int32 [n]): tgt_out[i] = out[i, target[i]]
hipError_t launch_log_softmax_rows(const float* logits, float* out, const int* target, float* tgt_out, int n, int V,
                                   hipStream_t st);
// out fp64 [n_var]: out[v] = sum, r ascending in [var_off[v], var_off[v+1]), of the fp32 difference lp[r,mt[r]] - lp[r,wt[r]], added
// in fp64 by one lane per variant (no atomics); lp fp32 [n_rows,V], columns clamped to [0,V), offsets to [0,n_rows]
hipError_t launch_score_rows(const float* lp, const int* wt, const int* mt, const int* var_off, double* out, int n_rows,
                             int n_var, int V, hipStream_t st);
// out fp64 [n_seq]: out[s] = sum, r ascending in [off[s], off[s+1]), of the fp32 lp[r,target[r]], added in fp64 by one lane per
// sequence (no atomics); target clamped to [0,V), offsets to [0,n_rows]
hipError_t launch_sum_target_rows(const float* lp, const int* target, const int* off, double* out, int n_rows, int n_seq, int V,
                                  hipStream_t st);
// windows.hip — proteins longer than the model's window (esm_amd/windows.py; the window copies are launch_copy_rows).
// out fp32 [n_out,E]: out[r] = (sum_k w[k] x[src[k]]) / sum_k w[k], k ascending in [off[r], off[r+1]), fp32, one lane per
// element; ONE entry: the row exactly; none: zeros; x [N,E] of any dtype code, E % 4 == 0, src clamped to [0,N)
hipError_t launch_blend_rows(const void* x, int x_dtype, const int* off, const int* src, const float* w, float* out, int N, int E,
                             int n_out, int total, hipStream_t st);
// out fp32 [Lb,Lb]: entry (i, j) from the window (maps [n_w,R,R], body start start[w] - body_lo) that holds both residues with
// the least |2 s + R - 1 - (i + j)|, ties to the lower start; NaN where no window holds both
hipError_t launch_stitch_contacts(const float* maps, const int* start, float* out, int n_w, int R, int Lb, int body_lo,
                                  hipStream_t st);
// sampling.hip — drawing sequences on the device (esm_amd/sampling.py).  Random numbers are Philox4x32-10 words addressed by
// key = seed and counter = (chain id, epoch or step, purpose, index); purpose 0 = permutation, 1 = token draw.
// perm_out[pos_off[c] : pos_off[c+1]] = Fisher-Yates shuffle of the same slice of pos_in (int32 [total]), one lane per chain;
// pos_off int32 [n_chain+1] (clamped to [0,total]; hi < lo: empty), chain_id int32 [n_chain]
hipError_t launch_permute_positions(const int* pos_off, const int* pos_in, const int* chain_id, int* perm_out, int n_chain,
                                    int total, unsigned long long seed, int epoch, hipStream_t st);
// one token per row of lp fp32 [n,V], V <= 64, from the candidates (bits of `allowed` below V, minus exclude[i]): tempered
// inverse-CDF draw with the uniform of counter (row_chain[i], step, 1, row_index[i]), or the argmax for inv_temperature == 0;
// token_out int32 [n] (-1: no candidate), logq_out fp32 [n], u_out fp32 [n] (optional); exclude int32 [n] (optional).
// A top-k / nucleus filter stands in front of the draw (rank by the fp32 inputs, fp32 weights added in rank order; top_k == 0
// and top_p == 1: off, the plain draw of esmk_op_sample_rows), and a per-row score over the unfiltered candidates goes with it
// (score_kind 0 none, 1 max log q, 2 sum q log q; fp64, rounded once); score_out fp32 [n], kept_out uint64 [n] (optional)
hipError_t launch_sample_rows(const float* lp, const int* row_chain, const int* row_index, const int* exclude,
                              unsigned long long allowed, float inv_temperature, unsigned long long seed, int step, int top_k,
                              float top_p, int score_kind, int* token_out, float* logq_out, float* u_out, float* score_out,
                              unsigned long long* kept_out, int n, int V, hipStream_t st);
// per chain c (rows row_off[c] : row_off[c+1] of score fp32 [n]) the sel_off[c+1] - sel_off[c] rows of the largest score, best
// first, into sel_out[sel_off[c] ..], the others in ascending row order into rest_out[rest_off[c] ..]; one workgroup per chain
hipError_t launch_select_rows(const float* score, const int* row_off, const int* sel_off, const int* rest_off, int* sel_out,
                              int* rest_out, int n_chain, int n, int n_sel, int n_rest, hipStream_t st);
// tokens[slot[i], pos[i]] = token[i] on int64 [B,T]; token < 0 or pos outside [0,T) writes nothing, slot clamped to [0,B)
hipError_t launch_commit_tokens(int64_t* tokens, const int* slot, const int* pos, const int* token, int n, int B, int T,
                                hipStream_t st);
// design.hip — Metropolis-Hastings design toward a target contact map (esm_amd/design.py).  Philox counters (chain id, step,
// purpose, 0): purpose 2 = proposal (words x: site, y: token), 3 = acceptance.  No atomics; one lane per chain except the energy.
// site = pos[pos_off[c] + mulhi32(x, len_c)], old = tokens[slot[c] or c, site], tok = set bit mulhi32(y, n_cand) of the candidates
// (bits of `allowed` below V, minus old with force_new); an empty list: site = old = tok = -1; no candidate: tok = -1
hipError_t launch_propose_mutations(const int64_t* tokens, const int* slot, const int* pos_off, const int* pos, const int* chain_id,
                                    unsigned long long allowed, int force_new, unsigned long long seed, int step, int* site_out,
                                    int* old_out, int* tok_out, int n_chain, int B, int T, int total, int V, hipStream_t st);
// energy[b] = -mean of log p over the target contacts (kind 0) or of y log p + (1 - y) log(1 - p) over the counted pairs (kind 1)
// of contacts fp32 [B,S,S] against target uint8 [S,S] (0 / 1 / 2 = ignore), pairs j - i >= min_sep; p clamped to [2^-24, 1 - 2^-24];
// fp64, one workgroup per chain, fixed order; count[b] = the terms, 0 terms: energy 0
hipError_t launch_contact_energy(const float* contacts, const unsigned char* target, double* energy_out, int* count_out, int B, int S,
                                 int min_sep, int kind, hipStream_t st);
// E' = (w_contact * e_contact[c] + w_lm * -(lp_sum[c] / n_res[c])) + w_extra * e_extra[c] (e_extra null: the sum of two); accept iff
// tok >= 0 and (a >= 0 or u < exp(a)), a = -(E' - e_cur[c]) * inv_t + hastings[c]; +inf: iff E' <= e_cur[c].  inv_t = inv_t0, or with
// a table (device fp64 [n_rung]) inv_t_tab[clamp(rung[c])] (rung null: entry 0).  On acceptance the token, e_cur and the
// component energies are written
hipError_t launch_mh_accept(int64_t* tokens, const int* slot, const int* site, const int* tok, const int* chain_id,
                            const double* e_contact, const double* lp_sum, const int* n_res, const double* hastings,
                            const double* e_extra, double w_contact, double w_lm, double w_extra, const double* inv_t_tab,
                            double inv_t0, const int* rung, int n_rung, unsigned long long seed, int step, double* e_cur,
                            double* e_contact_cur, double* e_lm_cur, double* e_extra_cur, unsigned char* accepted_out, double* u_out,
                            double* e_prop_out, int n_chain, int B, int T, hipStream_t st);
// h[c] = (double)inv_t_prop * ((double)lp[c, old[c]] - (double)lp[c, new[c]]); a token outside [0,V): 0
hipError_t launch_hastings_rows(const float* lp, const int* old_tok, const int* new_tok, float inv_t_prop, double* h_out, int n, int V,
                                hipStream_t st);
// tempering.hip — the n-gram term of the design energy and replica exchange (esm_amd/design.py).  fp64, no atomics.
// q[n - 1]: the dense background table fp64 [A^n] of order n (device memory), null for an order that is not chosen
struct NgramTables {
    const double* q[4];
};
// energy[b] = sum over the orders n of order_mask (bit n - 1), ascending, of KL_n = sum over the distinct keys of the chain's valid
// windows of p log(p / q_n[key]); tokens int64 [B,T], residues first .. first + S - 1, code int32 [V] (-1: outside the alphabet of
// A <= 32 letters; such a window is left out); one workgroup per chain, fixed order; S <= 32768
hipError_t launch_ngram_energy(const int64_t* tokens, const int* code, const NgramTables& q, double* energy_out, int B, int T,
                               int first, int S, int V, int A, int order_mask, hipStream_t st);
// (the acceptance with a temperature per chain and a third energy term is launch_mh_accept, design.hip)
// swap round `round` of n_ladder ladders of K consecutive slots: the chains at rungs k and k + 1, k % 2 == round % 2, exchange
// their rungs iff a >= 0 or u < exp(a), a = (inv_t[k] - inv_t[k+1]) * (e_cur[x] - e_cur[y]), u at counter (ladder_id, round, 4, k)
hipError_t launch_replica_swap(int* rung, const double* e_cur, const double* inv_t, const int* ladder_id, unsigned long long seed,
                               int round, unsigned char* accepted_out, double* u_out, int n_ladder, int K, hipStream_t st);
// jacobian.hip — the categorical Jacobian J[i,a,j,b] fp32 [L,nA,L,nA] of one protein (esm_amd/jacobian.py); nA <= 32, every
// index into J 64 bit, every sum fp64 in a fixed order, no atomics.  (The substituted copies are launch_copy_rows.)
// out [n_copies,L,nA] (the slice of J at the chunk's first copy): out[c,j,b] = logits[c*L+j, cols[b]] - wt[j, cols[b]] in fp32;
// logits fp32 [n_copies*L,V], wt fp32 [L,V], cols int32 [nA] clamped to [0,V)
hipError_t launch_jacobian_scatter(const float* logits, const float* wt, const int* cols, float* out, int n_copies, int L, int nA,
                                   int V, hipStream_t st);
// in place, four passes in the order b, j, a, i: x = (float)((double)x - mean), mean = the fp64 sum of the fp32 line in ascending
// index order / n
hipError_t launch_jacobian_center(float* J, int L, int nA, hipStream_t st);
// S fp32 [L,L]: S[i,j] = S[j,i] = sqrt(sum_ab (0.5 (Jc[i,a,j,b] + Jc[j,b,i,a]))^2), fp64 terms in a fixed order, rounded once
hipError_t launch_jacobian_contacts(const float* Jc, float* S, int L, int nA, hipStream_t st);
// in place on S fp32 [L,L]: diagonal := 0, S[i,j] -= r_i c_j / s (fp64 row, column and total sums; s == 0: no correction);
// work: 2 L + 1 doubles
hipError_t launch_apc(float* S, double* work, int L, hipStream_t st);
// contact head (modules.py:27-41,338-357)
hipError_t launch_contacts(const float* attn, const int64_t* tokens, const float* w,
                           const float* b, float* scratch, float* out, int B, int C, int T,
                           int eos_idx, int prepend_bos, int append_eos, hipStream_t st);

// contacts.hip — contact maps without the [B,L,H,T,T] attention tensor (predict_contacts, esm2.py:146-147).
// Per layer, after the attention kernel (q, k, lse still in the workspace): A[G][B,T,T] += sum_h w[layer,h] P_h
// (G = contacts_head_groups(B ceil(T/128)^2, H) accumulators, one per head group), rowsum / colsum [B,C,T] (C = L*H) masked sums
// of every channel; rowp [B, ceil(T/128), H, T] and colp [B, ceil(T/32), H, T] are per-layer scratch.
// pairs: (128-query block, 128-key chunk) pairs of the batch, B ceil(T/128)^2 padded (see contacts.hip)
int contacts_head_groups(long long pairs, int H, int head_dim);
hipError_t launch_contacts_fused_layer(const void* q, const void* k, const float* lse, const float* key_bias,
                                       const int64_t* tokens, const float* wreg, float* acc, float* rowsum,
                                       float* colsum, float* rowp, float* colp, int B, int H, int T, int C, int layer,
                                       int head_dim, int pad_idx, int eos_idx, int prepend_bos, int append_eos,
                                       int operand_dtype, hipStream_t st, int G = 0);
// after the last layer: rowsum becomes r_c (in place), wt [B,C] = w_c / t_c, out [B,S,S] = sigmoid(logits)
// G: 0 = contacts_head_groups(); otherwise the head-group count the layers ran with (esmk_op_contacts_fused_ex), which
// must hold a head in every group: G == ceil(H / ceil(H / G))
hipError_t launch_contacts_fused_final(const float* acc, float* rowsum, const float* colsum, float* wt,
                                       const int64_t* tokens, const float* wreg, const float* bias, float* out,
                                       int B, int H, int C, int T, int head_dim, int pad_idx, int eos_idx,
                                       int prepend_bos, int append_eos, hipStream_t st, int G = 0);

// Token-packed batch with contacts (esmk_forward_packed_ex): the same device code as the padded launchers above — each
// computation is one body in the coordinates of one sequence (contacts.hip), the two layouts differ in the kernels'
// prologues (where the workgroup's sequence and its scratch are) and in two strides.  Only segments with
// S = len - bos - eos > 0 get work and scratch.  Per segment s, element offsets off[4s..4s+3] (int64) into: one head group's accumulator (the G
// accumulators are [G][sum len^2]), rowp ([ceil(len/128), H, len] per segment), colp ([ceil(len/32), H, len]), and
// the ragged output (segment s's [S_s,S_s] map at sum_{s'<s} S_s'^2).  rowsum / colsum are [C, len] at C * (first
// row of s), wt [n_seg, C].  The work lists of the four kernels follow the offsets in one int32 table:
//   off [n_seg][8 int32] | accumulate [n_acc][4] (segment, key chunk, query block, 0), longest segments first |
//   reduce [n_red][2] (segment, 256-row block) | rt [n_rt] (segment) | final [n_fin][4] (segment, tile i, tile j, 0)
struct CtSegs {  // kernel argument of the packed contact kernels
    const int* seg = nullptr;        // [n_seg][2] (first row, length)
    const long long* off = nullptr;  // [n_seg][4]
    const int* work = nullptr;       // this launch's work list
    long long acc_stride = 0;        // elements of one head-group accumulator: sum of len^2
    int rows = 0, n_items = 0;       // row space of q / k / lse ([H, rows]); items of `work`
};
struct CtPackedPlan {
    int n_seg = 0, G = 1;
    long long sum_len2 = 0, rowp = 0, colp = 0, out = 0;  // elements
    long long n_acc = 0, n_red = 0, n_rt = 0, n_fin = 0;  // work items
    size_t table_ints() const { return 8 * (size_t)n_seg + 4 * n_acc + 2 * n_red + n_rt + 4 * n_fin; }
};
struct CtPackedDev {  // the table above on the device
    const int* seg = nullptr;
    const long long* off = nullptr;
    const int *acc_work = nullptr, *red_work = nullptr, *rt_work = nullptr, *fin_work = nullptr;
    int rows = 0;
};
CtPackedPlan contacts_packed_plan(const int32_t* seg, int n_seg, int H, int head_dim, int bos, int eos);
// dst: plan.table_ints() int32, 8-byte aligned
void contacts_packed_tables(const CtPackedPlan& p, const int32_t* seg, int bos, int eos, int H, int32_t* dst);
hipError_t launch_contacts_packed_layer(const void* q, const void* k, const float* lse, const float* key_bias,
                                        const int64_t* tokens, const float* wreg, float* acc, float* rowsum,
                                        float* colsum, float* rowp, float* colp, const CtPackedPlan& p,
                                        const CtPackedDev& d, int H, int C, int layer, int head_dim, int pad_idx,
                                        int eos_idx, int prepend_bos, int append_eos, int operand_dtype,
                                        hipStream_t st);
hipError_t launch_contacts_packed_final(const float* acc, float* rowsum, const float* colsum, float* wt,
                                        const int64_t* tokens, const float* wreg, const float* bias, float* out,
                                        const CtPackedPlan& p, const CtPackedDev& d, int C, int pad_idx, int eos_idx,
                                        int prepend_bos, int append_eos, hipStream_t st);

// token-packed batch (esmk_forward_packed): per-row bookkeeping of the packed row space.  Segment s occupies
// rows [seg[2s], seg[2s] + seg[2s+1]); rows outside every segment are gaps.
//   scale_row[m] = 1 - n_mask/len of m's segment (esm2.py:91-92; 1 in gaps), key_bias[m] = 0 / -inf (pad, gap),
//   row_pos[m] = m - segment start (0 in gaps), seg_npad[s] = number of <pad> tokens inside segment s
hipError_t launch_packed_stats(const int64_t* tokens, const int* seg, int n_seg, int rows, int pad_idx,
                               int mask_idx, float* scale_row, float* key_bias, int* row_pos, int* seg_npad,
                               hipStream_t st, float* keep = nullptr);  // keep[m] = 1 - pad (0 in gaps), optional

// rows outside every segment of buf[rows][row_bytes] := 0 (the attention kernel does not write them)
hipError_t launch_zero_gap_rows(void* buf, const int* seg, int n_seg, int rows, size_t row_bytes, hipStream_t st);

// ---- attention.hip ---------------------------------------------------------------------
// toolchain guard: the inline-asm MFMA of common.h (mma_keep_c) against the builtin; a, b [64 lanes][8] operand dtype,
// c [64][16] fp32, out [3][64][16] = {asm path, builtin path, C after the calls}
hipError_t launch_mma_keep_c_selftest(const void* a, const void* b, const float* c, float* out, int operand_dtype,
                                      hipStream_t st);
// query-block work list of a token-packed batch: work[4i..4i+3] = (first row of the segment, segment length,
// first query of block i relative to the segment, segment index); npad[s] = <pad> tokens inside segment s
struct AttnSegs {
    const int* work = nullptr;
    const int* npad = nullptr;
};
// lse: nullptr, or [H, rows] row log-sum-exp (log2 domain) for the packed contact kernels
hipError_t launch_attention_packed(const void* q, const void* k, const void* vt, const float* key_bias, void* ctx,
                                   float* lse, int H, int rows, int Tp, AttnSegs segs, int n_items, int operand_dtype,
                                   hipStream_t st);
hipError_t launch_attention128_packed(const void* q, const void* k, const void* vt, const float* key_bias, void* ctx,
                                      float* lse, int H, int rows, int Tp, AttnSegs segs, int n_items,
                                      int operand_dtype, hipStream_t st);
// Attention maps of a token-packed batch (attn_probs_packed_kernel / attn_probs128_packed_kernel): one workgroup per
// (work item, head).  q, k [H, rows, head_dim], lse [H, rows], key_bias [rows] (read only for segments with npad > 0).
// Ragged output: segment s owns a [Ltot, H, len_s, len_s] block at element offset Ltot * H * map_off[s], map_off[s] =
// sum_{s'<s} len_s'^2 (64-bit: four 650M sequences of 1022 tokens are already 2.8e9 elements).  lowp: maps in the operand
// dtype.  Every element carries the bits attn_probs_kernel gives the same sequence in a padded batch: the four map kernels
// (head_dim 64 / 128, padded / packed; all in attention.hip) are wrappers of one loop, attn_probs_rows<HD>.
hipError_t launch_attention_probs_packed(const void* q, const void* k, const float* lse, const float* key_bias, void* probs,
                                         int H, int rows, int layer, int num_layers_total, AttnSegs segs,
                                         const unsigned long long* map_off, int n_items, int operand_dtype, bool lowp,
                                         hipStream_t st);
hipError_t launch_attention_probs128_packed(const void* q, const void* k, const float* lse, const float* key_bias,
                                            void* probs, int H, int rows, int layer, int num_layers_total, AttnSegs segs,
                                            const unsigned long long* map_off, int n_items, int operand_dtype, bool lowp,
                                            hipStream_t st);
// npad[s] = number of rows of segment s (seg [n_seg][2] = first row, length) whose key_bias is not 0; key_bias null: all 0.
// What launch_packed_stats derives from the tokens, for callers that hold key_bias only (esmk_op_attention_packed)
hipError_t launch_seg_npad(const float* key_bias, const int* seg, int n_seg, int* npad, hipStream_t st);
// ctx rows ([rows, row_bytes]) and lse ([H, rows], optional) of segments with npad == length := 0 (esmk_op_attention_packed)
hipError_t launch_zero_allpad_segments(void* ctx, float* lse, const int* seg, const int* npad, int n_seg, int H, int rows,
                                       size_t row_bytes, hipStream_t st);
hipError_t launch_attention(const void* q, const void* k, const void* vt, const float* key_bias,
                            const int* seq_info, void* ctx, float* lse, int B, int H, int T, int Tp,
                            int operand_dtype, hipStream_t st);
hipError_t launch_attention_x3(const void* q, const void* k, const void* vt, const float* key_bias, const int* seq_info, void* ctx3,
                               float* lse, int B, int H, int T, int Tp, int operand_dtype, hipStream_t st);
// ESM-1 (add_bias_kv): the same padded-batch kernel with one learned null key / value pair per head, bias_k / bias_v [H, 64] in
// the operand dtype (bias_k unscaled); ctx and lse include it (attn_fwd_kernel NK)
hipError_t launch_attention_biaskv(const void* q, const void* k, const void* vt, const float* key_bias, const int* seq_info,
                                   const void* bias_k, const void* bias_v, void* ctx, float* lse, int B, int H, int T, int Tp,
                                   int operand_dtype, hipStream_t st);
// attention128.hip: head_dim 128 (esm2_t48_15B)
hipError_t launch_attention128(const void* q, const void* k, const void* vt, const float* key_bias,
                               const int* seq_info, void* ctx, float* lse, int B, int H, int T, int Tp,
                               int operand_dtype, hipStream_t st);
// attention maps at head_dim 128 (attention.hip, next to the head_dim-64 ones).  lowp: the maps are written in the operand
// dtype (probs points to fp16 / bf16 storage)
hipError_t launch_attention_probs128(const void* q, const void* k, const float* lse, const float* key_bias,
                                     float* probs, int B, int H, int T, int layer, int num_layers_total,
                                     int operand_dtype, hipStream_t st, bool lowp = false);
// same kernel, MSA column attention: key_fill[b,t] != 0 REPLACES the score by -10000 (masked_fill,
// axial_attention.py:211-215) and is only applied when any_pad[0] != 0
hipError_t launch_attention_fill(const void* q, const void* k, const void* vt, const float* key_fill,
                                 const int* any_pad, void* ctx, float* lse, int B, int H, int T, int Tp,
                                 int operand_dtype, hipStream_t st);
// col_attentions[b, layer, h, c, i, j] (msa_transformer.py:193-194) from q, k and the saved log-sum-exp
hipError_t launch_attention_probs_msa(const void* q, const void* k, const float* lse, const float* key_fill,
                                      const int* any_pad, float* probs, int Bmsa, int C, int H, int R,
                                      int layer, int num_layers_total, int operand_dtype, hipStream_t st);
hipError_t launch_attention_probs(const void* q, const void* k, const float* lse,
                                  const float* key_bias, float* probs, int B, int H, int T,
                                  int layer, int num_layers_total, int operand_dtype,
                                  hipStream_t st, bool lowp = false);

// pair_head.hip — linear pairwise heads on the attention maps (esmk_set_pair_head, esmk_op_pair_head).  q, k [L,B,H,T,head_dim]
// and lse [L,B,H,T] (log2 domain) of every layer, key_bias [B,T] (0 / -inf) and tokens [B,T] or null (either marks <pad>), w64 [L*H][64] (launch_pair_head_pad_w of
// w [L*H][n_sym + n_asym]), bias [n_sym + n_asym] or null; out fp32 [B,S,S,n_sym + n_asym], S = T - prepend_bos - append_eos:
// one accumulate launch over all channels, one in-place launch for the transpose term and the bias
hipError_t launch_pair_head_pad_w(const float* w, float* w64, int C, int C_out, hipStream_t st);
hipError_t launch_pair_head(const void* q, const void* k, const float* lse, const float* key_bias, const int64_t* tokens,
                            const float* w64, const float* bias, float* out, int L, int B, int H, int T, int head_dim, int n_sym,
                            int n_asym, int pad_idx, int prepend_bos, int append_eos, int operand_dtype, hipStream_t st);
// the categorical cross-entropy of n_bins logits at pair_logits[b,i,j,first ..] (row stride ld) against target uint8 [S,S]
// (>= n_bins: ignored), fp64, one workgroup per chain (esmk_op_distogram_energy)
hipError_t launch_distogram_energy(const float* logits, int ld, int first, int n_bins, const unsigned char* target,
                                   double* energy_out, int* count_out, int B, int S, int min_sep, double inv_temp,
                                   hipStream_t st);

}  // namespace esmk
