// engine_ops.hip — the single-kernel and debug entry points of libesmk.so (declared in include/esmk.h): validation,
// then the launchers the engines use themselves.  Tests and tools call these; esmk_forward / esmk_msa_forward do not.
#include "engine_internal.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

using namespace esmk;
using namespace esmk_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// single-kernel entry points
// ---------------------------------------------------------------------------------------------
// LayerNorm has two kernel forms (elementwise.hip).  Bits 8..11 of operand_dtype: 0 = default (the engine's form), else
// variant + 1 with variant 0 = the plain form and 7 = the engine's; variants 1 .. 6 were experiments that are gone.
static bool ln_form_ok(int operand_dtype) {
    const int sel = (operand_dtype >> 8) & 0xf;
    return sel == 0 || sel == 1 || sel == 8;
}

int esmk_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev,
                      void* y_dev, float* y32_dev, int rows, int E, int operand_dtype,
                      void* stream) {
    if (!ln_form_ok(operand_dtype)) return fail("esmk_op_layernorm: variant must be default, 0 or 7 (operand_dtype bits 8..11 = variant + 1)");
    ESMK_TRY(launch_layernorm(x_dev, gamma_dev, beta_dev, y_dev, y32_dev, rows, E, operand_dtype,
                              (hipStream_t)stream));
    return 0;
}

int esmk_op_masked_row_mean(const void* x_dev, int x_dtype, const int32_t* count_dev, float* out_dev, int B, int T,
                            int E, int first_row, void* stream) {
    if (!x_dev || !count_dev || !out_dev) return fail("esmk_op_masked_row_mean: null argument");
    if (B <= 0 || T <= 0 || E <= 0 || E % 4 != 0 || first_row < 0 || first_row > T)
        return fail("esmk_op_masked_row_mean: need B, T > 0, E a positive multiple of 4, 0 <= first_row <= T");
    if (x_dtype != ESMK_DT_F32 && x_dtype != ESMK_DT_F16 && x_dtype != ESMK_DT_BF16)
        return fail("esmk_op_masked_row_mean: x_dtype must be ESMK_F32, ESMK_F16 or ESMK_BF16");
    ESMK_TRY(launch_masked_row_mean(x_dev, x_dtype, count_dev, out_dev, B, T, E, first_row, (hipStream_t)stream));
    return 0;
}

int esmk_op_linear(const void* a_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                   int M, int N, int K, int epilogue, int operand_dtype, void* stream) {
    if (epilogue < 0 || epilogue > 4) return fail("esmk_op_linear: bad epilogue");
    GemmArgs g;
    g.A = a_dev;
    g.W = w_dev;
    g.bias = bias_dev;
    g.out = out_dev;
    g.M = M;
    g.N = N;
    g.K = K;
    if (operand_dtype & 0x100) g.force_generic = 1;  // test hook: force the generic 64x64 kernel
    if (operand_dtype & 0x200) g.force_old = 1;      // test hook: one-tile-per-workgroup 256x256 kernel
    g.panel_c = (operand_dtype >> 20) & 0x3f;         // tile-order experiments (tools/microbench.py)
    g.half_m = ((operand_dtype >> 28) & 3) == 1 ? 1 : (((operand_dtype >> 28) & 3) == 2 ? -1 : 0);  // 128-row tiles: force / never
    if (operand_dtype & 0xff000) return fail("esmk_op_linear: bits 12..19 of operand_dtype must be 0 (they selected timing experiments that are gone)");
    operand_dtype &= 0xff;
    ESMK_TRY(launch_gemm(g, epilogue, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_op_split_weight(const void* w_dev, int w_dtype, void* w2_dev, int N, int K, void* stream) {
    if (!w_dev || !w2_dev) return fail("esmk_op_split_weight: null argument");
    if (N <= 0 || K <= 0 || K % 64 != 0) return fail("esmk_op_split_weight: need N > 0 and K a positive multiple of 64");
    ESMK_TRY(launch_convert2d_split(w_dev, w_dtype, w2_dev, (size_t)N, (size_t)K, (size_t)K, 0, 0, 64, (hipStream_t)stream));
    return 0;
}

int esmk_op_linear_split(const void* a_dev, const void* w2_dev, const float* bias_dev, void* out_dev, int M, int N, int K,
                         int epilogue, void* stream) {
    if (epilogue < 0 || epilogue > 4 || epilogue == EPI_GELU_F32) return fail("esmk_op_linear_split: epilogue must be 0, 1, 2 or 4");
    if (K % 64 != 0 || N % 8 != 0) return fail("esmk_op_linear_split: need K % 64 == 0 and N % 8 == 0");
    GemmArgs g;
    g.A = a_dev;
    g.W = w2_dev;
    g.bias = bias_dev;
    g.out = out_dev;
    g.M = M;
    g.N = N;
    g.K = 2 * K;
    g.a_row_bytes = (long long)K * 2;
    g.a_kt_repeat = 1;
    ESMK_TRY(launch_gemm(g, epilogue, ESMK_DT_F16, (hipStream_t)stream));
    return 0;
}

// ---- the kernels of the precision modes as single ops (tests/test_precision_ops_gpu.py) ---------------------------
int esmk_op_linear_f32(const float* a_dev, int lda, const float* w_dev, const float* bias_dev, float* out_dev, int ldc, int M,
                       int N, int K, int gelu, void* stream) {
    if (!a_dev || !w_dev || !out_dev) return fail("esmk_op_linear_f32: null argument");
    if (M <= 0 || N <= 0 || K <= 0) return fail("esmk_op_linear_f32: M, N and K must be positive");
    if (K % 32 != 0) return fail("esmk_op_linear_f32: need K % 32 == 0");
    if (lda % 4 != 0 || lda < K) return fail("esmk_op_linear_f32: need lda % 4 == 0 and lda >= K");
    if (ldc < N) return fail("esmk_op_linear_f32: need ldc >= N");
    ESMK_TRY(launch_gemm32(a_dev, lda, w_dev, bias_dev, out_dev, ldc, M, N, K, gelu != 0, (hipStream_t)stream));
    return 0;
}

int esmk_op_layernorm_ex(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, float* y32_dev,
                         int rows, int E, int operand_dtype, const float* row_keep_dev, int map_R, int map_C, int ldy, int x3,
                         float eps, void* stream) {
    if (!ln_form_ok(operand_dtype)) return fail("esmk_op_layernorm_ex: variant must be default, 0 or 7 (operand_dtype bits 8..11 = variant + 1)");
    if (!x_dev || !gamma_dev || !beta_dev || (!y_dev && !y32_dev)) return fail("esmk_op_layernorm_ex: null argument");
    if (rows <= 0 || E <= 0) return fail("esmk_op_layernorm_ex: rows and E must be positive");
    if (E % 4 != 0 || E > 5120) return fail("esmk_op_layernorm_ex: need E % 4 == 0 and E <= 5120");
    const int dt = operand_dtype & 0xff;
    if (dt != ESMK_DT_F16 && dt != ESMK_DT_BF16) return fail("esmk_op_layernorm_ex: operand_dtype must be ESMK_F16 or ESMK_BF16");
    if (ldy < 0 || (ldy > 0 && ldy < E) || ldy % 4 != 0) return fail("esmk_op_layernorm_ex: ldy must be 0 or a multiple of 4 >= E");
    if (x3 && (E % 64 != 0 || ldy < 3 * E || !y_dev || dt != ESMK_DT_F16))
        return fail("esmk_op_layernorm_ex: x3 needs E % 64 == 0, ldy >= 3 E, y and fp16");
    if (map_R < 0 || (map_R > 0 && (map_C <= 0 || rows % ((long long)map_R * map_C) != 0)))
        return fail("esmk_op_layernorm_ex: the row map needs map_C > 0 and rows % (map_R map_C) == 0");
    if (!(eps > 0.f)) return fail("esmk_op_layernorm_ex: eps must be positive");
    LnExtra ex;
    ex.row_keep = row_keep_dev;
    ex.map_R = map_R;
    ex.map_C = map_R > 0 ? map_C : 0;
    ex.ldy = ldy;
    ex.x3 = x3 != 0;
    ex.eps = eps;
    ESMK_TRY(launch_layernorm_ex(x_dev, gamma_dev, beta_dev, y_dev, y32_dev, rows, E, operand_dtype, ex, (hipStream_t)stream));
    return 0;
}

int esmk_op_split_weight_ex(const void* w_dev, int w_dtype, void* dst_dev, int dst_dtype, int rows, int cols, int dst_ld,
                            int parts, int row_map, int col_map, int head_dim, void* stream) {
    auto is_dt = [](int d) { return d == ESMK_DT_F32 || d == ESMK_DT_F16 || d == ESMK_DT_BF16; };
    if (!w_dev || !dst_dev) return fail("esmk_op_split_weight_ex: null argument");
    if (rows <= 0 || cols <= 0) return fail("esmk_op_split_weight_ex: rows and cols must be positive");
    if (parts < 1 || parts > 3) return fail("esmk_op_split_weight_ex: parts must be 1, 2 or 3");
    if (!is_dt(w_dtype) || !is_dt(dst_dtype)) return fail("esmk_op_split_weight_ex: dtypes must be ESMK_F32, ESMK_F16 or ESMK_BF16");
    if (parts >= 2 && dst_dtype != ESMK_DT_F16) return fail("esmk_op_split_weight_ex: parts 2 and 3 write fp16 (dst_dtype ESMK_F16)");
    if ((row_map != 0 && row_map != 1) || (col_map != 0 && col_map != 1))
        return fail("esmk_op_split_weight_ex: row_map and col_map must be 0 or 1");
    int d = 64;  // identity maps: unused
    if (row_map || col_map) {
        d = head_dim;
        if (!((d >= 1 && d <= 64) || d == 128)) return fail("esmk_op_split_weight_ex: head_dim must be 1..64 or 128");
        if ((row_map && rows % d != 0) || (col_map && cols % d != 0))
            return fail("esmk_op_split_weight_ex: head_dim must divide the mapped extent");
    }
    const long long col_extent = !col_map ? cols : d == 128 ? cols : (long long)(cols / d) * 64;
    if (dst_ld < col_extent) return fail("esmk_op_split_weight_ex: dst_ld is smaller than the (mapped) column extent");
    if (parts >= 2 && dst_ld % 64 != 0) return fail("esmk_op_split_weight_ex: parts 2 and 3 need dst_ld % 64 == 0");
    if (parts == 1)
        ESMK_TRY(launch_convert2d(w_dev, w_dtype, dst_dev, dst_dtype, (size_t)rows, (size_t)cols, (size_t)dst_ld, row_map, col_map,
                                  d, (hipStream_t)stream));
    else
        ESMK_TRY(launch_convert2d_split(w_dev, w_dtype, dst_dev, (size_t)rows, (size_t)cols, (size_t)dst_ld, row_map, col_map, d,
                                        (hipStream_t)stream, parts));
    return 0;
}

int esmk_op_linear_gelu_x3(const void* a3_dev, const void* w3_dev, const float* bias_dev, void* out3_dev, int M, int N, int K3,
                           void* stream) {
    if (!a3_dev || !w3_dev || !bias_dev || !out3_dev) return fail("esmk_op_linear_gelu_x3: null argument");
    if (M <= 0 || N <= 0 || K3 <= 0) return fail("esmk_op_linear_gelu_x3: M, N and K3 must be positive");
    if (K3 % 192 != 0) return fail("esmk_op_linear_gelu_x3: need K3 % 192 == 0 (hi | hi | lo per 64-column K tile)");
    GemmArgs g;
    g.A = a3_dev;
    g.W = w3_dev;
    g.bias = bias_dev;
    g.out = out3_dev;
    g.M = M;
    g.N = N;
    g.K = K3;
    g.x3_out = 1;
    // the kernel's own contract (gemm9_supports): a 64-column block is stored as hi | hi | lo, 192 columns of a 3 N row
    if (N % 64 != 0 || gemm_plan(g, EPI_GELU_T).kernel != 9)
        return fail("esmk_op_linear_gelu_x3: need N % 64 == 0 (no kernel takes this call)");
    ESMK_TRY(launch_gemm(g, EPI_GELU_T, ESMK_DT_F16, (hipStream_t)stream));
    return 0;
}

int esmk_debug_linear_splitk(const void* a_dev, const void* w_dev, float* partials_dev, int M, int N, int K,
                             int S, int operand_dtype, void* stream) {
    if (S < 1 || K % S != 0 || (K / S) % 64 != 0) return fail("esmk_debug_linear_splitk: K/S must be a multiple of 64");
    GemmArgs g;
    g.A = a_dev;
    g.W = w_dev;
    g.out = partials_dev;
    g.M = M;
    g.N = N;
    g.K = K / S;
    g.a_row_bytes = g.w_row_bytes = (long long)K * 2;  // rows keep the full-K stride
    g.batch = S;
    g.a_bo = g.w_bo = (long long)(K / S) * 2;           // slice s starts K/S operand elements further right
    g.o_bo = (long long)M * N * 4;
    ESMK_TRY(launch_gemm(g, EPI_STORE_F32, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_debug_gemm_timing(void* stamps_dev) {
    gemm8_set_timing((unsigned long long*)stamps_dev);
    gemm9_set_timing((unsigned long long*)stamps_dev);
    return 0;
}

int esmk_debug_mma_selftest(const void* a_dev, const void* b_dev, const float* c_dev, float* out_dev, int operand_dtype,
                            void* stream) {
    if (!a_dev || !b_dev || !c_dev || !out_dev) return fail("esmk_debug_mma_selftest: null argument");
    ESMK_TRY(launch_mma_keep_c_selftest(a_dev, b_dev, c_dev, out_dev, operand_dtype, (hipStream_t)stream));
    return 0;
}

// ---- LayerNorm fold as single ops (tests/test_ln_fold_gpu.py) ----------------------------------------------------
int esmk_op_rowstats(const float* x_dev, void* y_dev, float* mean_dev, float* rstd_dev, int rows, int E, int ldy,
                     int operand_dtype, void* stream) {
    if (!x_dev || !y_dev || !mean_dev || !rstd_dev) return fail("esmk_op_rowstats: null argument");
    ESMK_TRY(launch_rowstats(x_dev, y_dev, mean_dev, rstd_dev, rows, E, ldy, operand_dtype, (hipStream_t)stream));
    return 0;
}

// ---- one edit of the residual stream as a single op (tests/test_stream_edit_ops_gpu.py) --------------------------
int esmk_op_stream_edit(float* x_dev, const int64_t* tokens_dev, int N, int E, const esmk_stream_edit* edit, void* y_dev, int ldy,
                        float* mean_dev, float* rstd_dev, int operand_dtype, void* stream) {
    if (!x_dev || !edit) return fail("esmk_op_stream_edit: null argument");
    if (N <= 0 || N > ESMK_MAX_ROWS || E <= 0) return fail("esmk_op_stream_edit: need 0 < N <= 2^24 and E > 0");
    if (check_stream_edit("esmk_op_stream_edit", *edit, E, -1)) return 1;
    if (!edit->rows_dev && !tokens_dev) return fail("esmk_op_stream_edit: the token selector (rows_dev NULL) needs tokens_dev");
    if (y_dev && (!mean_dev || !rstd_dev)) return fail("esmk_op_stream_edit: the fold outputs are y_dev, mean_dev and rstd_dev together");
    if (y_dev && (ldy < E || ldy % 4 != 0)) return fail("esmk_op_stream_edit: ldy must be a multiple of 4 that is >= E");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_stream_edit: operand_dtype must be ESMK_F16 or ESMK_BF16");
    StreamEditArgs a = stream_edit_args(*edit, x_dev, tokens_dev, N, E);
    a.y = y_dev;
    a.ldy = ldy;
    a.mean = mean_dev;
    a.rstd = rstd_dev;
    ESMK_TRY(launch_stream_edit(a, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_op_ln_finalize(const float* part_dev, float* mean_dev, float* rstd_dev, int rows, int parts, int E, void* stream) {
    if (!part_dev || !mean_dev || !rstd_dev) return fail("esmk_op_ln_finalize: null argument");
    ESMK_TRY(launch_ln_finalize(part_dev, mean_dev, rstd_dev, rows, parts, E, (hipStream_t)stream));
    return 0;
}

// the checks and the launch of both fold_weight entries; row_map: rows of heads of d dims spread over 64 slots
static int fold_weight_op(const void* w_dev, int w_dtype, const float* gamma_dev, const float* beta_dev, void* dst_dev,
                          int dst_dtype, float* bias2_dev, int N, int K, int ld, int row_map, int d, void* stream) {
    if (!w_dev || !gamma_dev || !beta_dev || !dst_dev || !bias2_dev) return fail("esmk_op_fold_weight: null argument");
    if (N <= 0 || K <= 0 || ld < K) return fail("esmk_op_fold_weight: need N, K > 0 and ld >= K");
    ESMK_TRY(launch_fold_weight(w_dev, w_dtype, gamma_dev, beta_dev, dst_dev, dst_dtype, bias2_dev, (size_t)N, (size_t)K,
                                (size_t)ld, row_map, d, (hipStream_t)stream));
    return 0;
}

int esmk_op_fold_weight_ex(const void* w_dev, int w_dtype, const float* gamma_dev, const float* beta_dev, void* dst_dev,
                           int dst_dtype, float* bias2_dev, int N, int K, int ld, int head_dim, void* stream) {
    if (head_dim != 16 && head_dim != 24 && head_dim != 32 && head_dim != 64)
        return fail("esmk_op_fold_weight_ex: head_dim must be 16, 24, 32 or 64");
    if (N > 0 && N % head_dim != 0) return fail("esmk_op_fold_weight_ex: need N % head_dim == 0 (whole heads)");
    return fold_weight_op(w_dev, w_dtype, gamma_dev, beta_dev, dst_dev, dst_dtype, bias2_dev, N, K, ld, head_dim < 64, head_dim,
                          stream);
}

// the entry without head_dim: the identity row map for any N (head_dim 64 without the whole-heads condition)
int esmk_op_fold_weight(const void* w_dev, int w_dtype, const float* gamma_dev, const float* beta_dev, void* dst_dev,
                        int dst_dtype, float* bias2_dev, int N, int K, int ld, void* stream) {
    return fold_weight_op(w_dev, w_dtype, gamma_dev, beta_dev, dst_dev, dst_dtype, bias2_dev, N, K, ld, 0, 64, stream);
}

int esmk_op_linear_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const float* bias2_dev, void* out_dev,
                      int M, int N, int K, int epilogue, int operand_dtype, const float* ln_rstd_dev, void* h16_dev, int ldh,
                      float* ln_part_dev, int ln_parts, const float* ln_mean_dev, int half_m, void* stream) {
    if (epilogue != EPI_GELU_T && epilogue != EPI_RESID_F32)
        return fail("esmk_op_linear_ln: epilogue must be 2 (consumer: gelu) or 4 (producer: residual)");
    GemmArgs g;
    g.A = a_dev;
    g.W = w_dev;
    g.bias = bias_dev;
    g.bias2 = bias2_dev;
    g.out = out_dev;
    g.M = M;
    g.N = N;
    g.K = K;
    g.half_m = half_m;
    if (epilogue == EPI_GELU_T) {
        if (!ln_rstd_dev || !bias_dev) return fail("esmk_op_linear_ln: the consumer needs ln_rstd and bias");
        g.ln_rstd = ln_rstd_dev;
    } else {
        if (!h16_dev || !ln_part_dev || !ln_mean_dev) return fail("esmk_op_linear_ln: the producer needs h16, ln_part and ln_mean");
        g.h16 = h16_dev;
        g.ldh = ldh;
        g.ln_part = ln_part_dev;
        g.ln_parts = ln_parts;
        g.ln_mean = ln_mean_dev;
    }
    ESMK_TRY(launch_gemm(g, epilogue, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_debug_set(const char* key, double value) {
    if (!key) return fail("esmk_debug_set: null key");
    if (gemm_set_knob(key, value)) return 0;
    if (strcmp(key, "rows_contacts_own_groups") == 0) {
        g_rows_contacts_own_groups = value != 0.0;
        return 0;
    }
    return fail("esmk_debug_set: unknown key");
}

int esmk_debug_gemm_impl(int impl, int variant) {
    if (impl != 8 && impl != 9 && impl != 0) return fail("esmk_debug_gemm_impl: impl must be 8, 9 or 0 (automatic choice)");
    if (!gemm_set_impl(impl, variant))
        return fail("esmk_debug_gemm_impl: variant must be 0 (gemm9 has one form)");
    return 0;
}

int esmk_debug_gemm_plan(int M, int N, int K, int epilogue, int flags, int32_t out[4]) {
    if (!out) return fail("esmk_debug_gemm_plan: null argument");
    if (epilogue < EPI_STORE_T || epilogue > EPI_QKV_ALL) return fail("esmk_debug_gemm_plan: bad epilogue");
    if (flags & ~63) return fail("esmk_debug_gemm_plan: unknown flag");
    if ((flags & 32) && (flags != 32 || epilogue != EPI_GELU_T))
        return fail("esmk_debug_gemm_plan: the f16x3 output form (flag 32) exists for epilogue 2 alone, with no other flag");
    static const float fake = 0.f;  // stands for the pointers that select a form; gemm_plan dereferences nothing
    GemmArgs g;
    g.bias = &fake;
    g.M = M;
    g.N = N;
    g.K = K;
    if (epilogue == EPI_QKV_ALL) g.E = N % 3 == 0 ? N / 3 : 0;
    if (flags & 1) g.force_generic = 1;
    if (flags & 2) g.force_old = 1;
    if (flags & 4) {  // LayerNorm fold: producer form of the residual epilogue, consumer form of q / k, v, fc1
        if (epilogue == EPI_RESID_F32) g.ln_part = const_cast<float*>(&fake);
        else g.ln_rstd = &fake;
        if (!gemm9_ln_fold(g, epilogue)) return fail("esmk_debug_gemm_plan: this epilogue has no LayerNorm-fold form");
    }
    if (flags & 8) {  // as esmk_op_linear_split: the GEMM runs over the [N,2K] hi | lo image of the weight
        g.K = 2 * K;
        g.a_row_bytes = (long long)K * 2;
        g.a_kt_repeat = 1;
    }
    if (flags & 16) g.batch = 2;
    if (flags & 32) g.x3_out = 1;  // as esmk_op_linear_gelu_x3
    const GemmPlan pl = gemm_plan(g, epilogue);
    out[0] = pl.kernel;
    out[1] = pl.half_m;
    out[2] = 0;  // was: the gemm9 variant
    out[3] = 0;
    return 0;
}

static int qkv_rope_impl(esmk_model* m, const void* a_dev, const void* wqkv_dev, const float* bias_dev,
                         const float* bias2_dev, const float* ln_rstd_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                         int log2_domain, void* stream);

int esmk_op_qkv_rope2(esmk_model* m, const void* a_dev, const void* wqkv_dev,
                      const float* bias_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                      int log2_domain, void* stream) {
    return qkv_rope_impl(m, a_dev, wqkv_dev, bias_dev, nullptr, nullptr, q_out, k_out, vt_out, B, T, log2_domain, stream);
}

int esmk_op_qkv_rope_ln(esmk_model* m, const void* a_dev, const void* wqkv_dev, const float* bias_dev,
                        const float* bias2_dev, const float* ln_rstd_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                        int log2_domain, void* stream) {
    if (!ln_rstd_dev || !bias_dev) return fail("esmk_op_qkv_rope_ln: ln_rstd and bias are required");
    return qkv_rope_impl(m, a_dev, wqkv_dev, bias_dev, bias2_dev, ln_rstd_dev, q_out, k_out, vt_out, B, T, log2_domain, stream);
}

static int qkv_rope_impl(esmk_model* m, const void* a_dev, const void* wqkv_dev, const float* bias_dev,
                         const float* bias2_dev, const float* ln_rstd_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                         int log2_domain, void* stream) {
    if (!m) return fail("esmk_op_qkv_rope: null model");
    if (m->D != 64 || m->Kp != m->E) return fail("esmk_op_qkv_rope: single-op entry point needs head_dim 64");
    hipStream_t st = (hipStream_t)stream;
    if (ensure_rope(m, T, st)) return 1;
    const int Tp = (T + 63) / 64 * 64;
    if (Tp != T)
        ESMK_TRY(hipMemsetAsync(vt_out, 0, (size_t)B * m->H * 64 * Tp * op_size(m->cfg.operand_dtype),
                                st));
    QkvProj p;
    p.A = a_dev;
    p.K = m->E;
    p.W = wqkv_dev;
    p.bias = bias_dev, p.bias2 = bias2_dev, p.ln_rstd = ln_rstd_dev;
    p.q = q_out, p.k = k_out, p.vt = vt_out;
    p.cos = m->d_cos;
    p.sin = m->d_sin;
    p.rows = B * T, p.T = T, p.Tp = Tp;
    // log2_domain: q also carries log2(e), the form esmk_op_attention / esmk_op_attention_probs take (esmk_forward's own)
    p.scaling = (log2_domain ? kLog2e : 1.0f) / sqrtf((float)m->D);
    GemmArgs g, gv;
    qkv_gemm_args(m, p, &g, &gv);
    if (gemm_qkv_one_launch(g)) {  // as esmk_forward: one launch where it saves rounds of tiles
        g.N = 3 * m->E;
        ESMK_TRY(launch_gemm(g, EPI_QKV_ALL, m->cfg.operand_dtype, st));
        return 0;
    }
    ESMK_TRY(launch_gemm(g, EPI_QKV_ROPE, m->cfg.operand_dtype, st));
    ESMK_TRY(launch_gemm(gv, EPI_V_T, m->cfg.operand_dtype, st));
    return 0;
}

int esmk_op_qkv_rope(esmk_model* m, const void* a_dev, const void* wqkv_dev,
                     const float* bias_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                     void* stream) {
    return esmk_op_qkv_rope2(m, a_dev, wqkv_dev, bias_dev, q_out, k_out, vt_out, B, T, 0, stream);
}

int esmk_op_attention(const void* q_dev, const void* k_dev, const void* vt_dev,
                      const float* key_bias_dev, void* ctx_out, float* lse_out, int B, int H,
                      int T, int operand_dtype, void* stream) {
    const int Tp = (T + 63) / 64 * 64;
    ESMK_TRY(launch_attention(q_dev, k_dev, vt_dev, key_bias_dev, nullptr, ctx_out, lse_out, B, H, T,
                              Tp, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_op_attention_probs(const void* q_dev, const void* k_dev, const float* lse_dev,
                            const float* key_bias_dev, float* probs_out, int B, int H, int T,
                            int layer, int num_layers_total, int operand_dtype, void* stream) {
    ESMK_TRY(launch_attention_probs(q_dev, k_dev, lse_dev, key_bias_dev, probs_out, B, H, T, layer,
                                    num_layers_total, operand_dtype, (hipStream_t)stream));
    return 0;
}

// Every form of the attention core that esmk_forward / esmk_msa_forward launch, reachable one kernel at a time
// (tests/test_attention_variants_gpu.py).  Validation only, then the engine's own launchers.
int esmk_op_attention_ex(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                         const int32_t* seq_info_dev, const int32_t* any_pad_dev, void* ctx_out, float* lse_out, int B,
                         int H, int T, int Tp, int head_dim, int mode, int operand_dtype, void* stream) {
    if (!q_dev || !k_dev || !vt_dev || !ctx_out) return fail("esmk_op_attention_ex: null argument");
    if (B <= 0 || H <= 0 || T <= 0) return fail("esmk_op_attention_ex: B, H and T must be positive");
    if (Tp < T || Tp % 64 != 0) return fail("esmk_op_attention_ex: Tp must be a multiple of 64 and >= T");
    if (head_dim != 64 && head_dim != 128) return fail("esmk_op_attention_ex: head_dim must be 64 or 128");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_attention_ex: operand_dtype must be fp16 or bf16");
    if (mode < 0 || mode > 2) return fail("esmk_op_attention_ex: mode must be 0, 1 or 2");
    if (mode != 0 && head_dim != 64) return fail("esmk_op_attention_ex: modes 1 and 2 need head_dim 64");
    if (mode == 2 && operand_dtype != ESMK_DT_F16) return fail("esmk_op_attention_ex: mode 2 (f16x3) needs fp16");
    if (seq_info_dev && (mode == 1 || !key_bias_dev))
        return fail("esmk_op_attention_ex: seq_info needs key_bias and mode 0 or 2");
    if (any_pad_dev && mode != 1) return fail("esmk_op_attention_ex: any_pad belongs to mode 1");
    hipStream_t st = (hipStream_t)stream;
    if (head_dim == 128)
        ESMK_TRY(launch_attention128(q_dev, k_dev, vt_dev, key_bias_dev, seq_info_dev, ctx_out, lse_out, B, H, T, Tp,
                                     operand_dtype, st));
    else if (mode == 1)
        ESMK_TRY(launch_attention_fill(q_dev, k_dev, vt_dev, key_bias_dev, any_pad_dev, ctx_out, lse_out, B, H, T, Tp,
                                       operand_dtype, st));
    else if (mode == 2)
        ESMK_TRY(launch_attention_x3(q_dev, k_dev, vt_dev, key_bias_dev, seq_info_dev, ctx_out, lse_out, B, H, T, Tp,
                                     operand_dtype, st));
    else
        ESMK_TRY(launch_attention(q_dev, k_dev, vt_dev, key_bias_dev, seq_info_dev, ctx_out, lse_out, B, H, T, Tp,
                                  operand_dtype, st));
    return 0;
}

int esmk_op_attention_biaskv(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                             const int32_t* seq_info_dev, const void* bias_k_dev, const void* bias_v_dev, void* ctx_out,
                             float* lse_out, int B, int H, int T, int Tp, int operand_dtype, void* stream) {
    if (!q_dev || !k_dev || !vt_dev || !bias_k_dev || !bias_v_dev || !ctx_out) return fail("esmk_op_attention_biaskv: null argument");
    if (B <= 0 || H <= 0 || T <= 0) return fail("esmk_op_attention_biaskv: B, H and T must be positive");
    if (Tp < T || Tp % 64 != 0) return fail("esmk_op_attention_biaskv: Tp must be a multiple of 64 and >= T");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_attention_biaskv: operand_dtype must be fp16 or bf16");
    if (seq_info_dev && !key_bias_dev) return fail("esmk_op_attention_biaskv: seq_info needs key_bias");
    ESMK_TRY(launch_attention_biaskv(q_dev, k_dev, vt_dev, key_bias_dev, seq_info_dev, bias_k_dev, bias_v_dev, ctx_out, lse_out, B,
                                     H, T, Tp, operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_op_attention_probs_ex(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                               const int32_t* any_pad_dev, void* probs_out, int B, int H, int T, int head_dim, int layer,
                               int num_layers_total, int msa_C, int out_dtype, int operand_dtype, void* stream) {
    if (!q_dev || !k_dev || !lse_dev || !probs_out) return fail("esmk_op_attention_probs_ex: null argument");
    if (B <= 0 || H <= 0 || T <= 0) return fail("esmk_op_attention_probs_ex: B, H and T must be positive");
    if (head_dim != 64 && head_dim != 128) return fail("esmk_op_attention_probs_ex: head_dim must be 64 or 128");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_attention_probs_ex: operand_dtype must be fp16 or bf16");
    if (out_dtype != ESMK_DT_F32 && out_dtype != operand_dtype)
        return fail("esmk_op_attention_probs_ex: out_dtype must be fp32 or the operand dtype");
    if (layer < 0 || layer >= num_layers_total) return fail("esmk_op_attention_probs_ex: layer out of range");
    if (msa_C < 0) return fail("esmk_op_attention_probs_ex: msa_C must be >= 0");
    if (msa_C > 0 && (head_dim != 64 || out_dtype != ESMK_DT_F32 || B % msa_C != 0))
        return fail("esmk_op_attention_probs_ex: the MSA layout needs head_dim 64, fp32 maps and B a multiple of msa_C");
    if (any_pad_dev && msa_C == 0) return fail("esmk_op_attention_probs_ex: any_pad belongs to the MSA layout");
    hipStream_t st = (hipStream_t)stream;
    const bool lowp = out_dtype != ESMK_DT_F32;
    if (msa_C > 0)
        ESMK_TRY(launch_attention_probs_msa(q_dev, k_dev, lse_dev, key_bias_dev, any_pad_dev, (float*)probs_out, B / msa_C,
                                            msa_C, H, T, layer, num_layers_total, operand_dtype, st));
    else if (head_dim == 128)
        ESMK_TRY(launch_attention_probs128(q_dev, k_dev, lse_dev, key_bias_dev, (float*)probs_out, B, H, T, layer,
                                           num_layers_total, operand_dtype, st, lowp));
    else
        ESMK_TRY(launch_attention_probs(q_dev, k_dev, lse_dev, key_bias_dev, (float*)probs_out, B, H, T, layer,
                                        num_layers_total, operand_dtype, st, lowp));
    return 0;
}

// The packed attention core and the packed map kernel one kernel at a time (tests/test_attention_packed_ops_gpu.py).
// Validation first, before the HIP runtime is touched; then a work list of the entry's own — [seg 2 n][npad n][work 4 items]
// [map offsets uint64 n], the layout esmk_forward_packed_maps uploads — is built, uploaded, used and freed: no state stays.
namespace {
struct PackedOpTables {
    std::vector<int32_t> host;
    int n_items = 0;
    size_t map_base = 0;
    unsigned long long sum_len2 = 0;
};
struct DevBuf {  // freed on every way out of the entry
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
int packed_op_tables(const std::string& w, const int32_t* seg, int n_seg, int rows, PackedOpTables* t) {
    if (!seg) return fail(w + ": null segment table");
    SegTableInfo info;
    if (check_seg_table(w, seg, n_seg, rows, true, &info)) return 1;
    t->n_items = (int)info.items;
    t->sum_len2 = info.sum_len2;
    const PackedTables lay = packed_tables(n_seg, info.items, 0, true);
    t->map_base = lay.map_base;
    t->host.assign(lay.ints, 0);
    fill_attn_tables(seg, n_seg, t->host.data());
    fill_map_offsets(seg, n_seg, t->host.data() + t->map_base);
    return 0;
}
}  // namespace

int esmk_op_attention_packed(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                             const int32_t* segments_host, int n_seg, int rows, int Tp, int H, int head_dim,
                             int operand_dtype, const void* bias_k_dev, const void* bias_v_dev, void* ctx_out, float* lse_out,
                             void* stream) {
    const std::string w("esmk_op_attention_packed");
    if (!q_dev || !k_dev || !vt_dev || !ctx_out) return fail(w + ": null argument");
    if (bias_k_dev || bias_v_dev)
        return fail(w + ": bias_k / bias_v must be null (the null key of the ESM-1 models has no token-packed form)");
    if (H <= 0) return fail(w + ": H must be positive");
    if (head_dim != 64 && head_dim != 128) return fail(w + ": head_dim must be 64 or 128");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16) return fail(w + ": operand_dtype must be fp16 or bf16");
    PackedOpTables t;
    if (packed_op_tables(w, segments_host, n_seg, rows, &t)) return 1;
    if (Tp % 64 != 0 || Tp < rows + 64) return fail(w + ": Tp must be a multiple of 64 and >= rows + 64 (one spare key tile)");
    hipStream_t st = (hipStream_t)stream;
    DevBuf d;
    ESMK_TRY(hipMalloc(&d.p, t.host.size() * 4));
    ESMK_TRY(hipMemcpy(d.p, t.host.data(), t.host.size() * 4, hipMemcpyHostToDevice));
    int* tab = (int*)d.p;
    AttnSegs segs;
    segs.npad = tab + (size_t)2 * n_seg;
    segs.work = tab + (size_t)3 * n_seg;
    ESMK_TRY(launch_seg_npad(key_bias_dev, tab, n_seg, tab + (size_t)2 * n_seg, st));
    if (head_dim == 128)
        ESMK_TRY(launch_attention128_packed(q_dev, k_dev, vt_dev, key_bias_dev, ctx_out, lse_out, H, rows, Tp, segs, t.n_items,
                                            operand_dtype, st));
    else
        ESMK_TRY(launch_attention_packed(q_dev, k_dev, vt_dev, key_bias_dev, ctx_out, lse_out, H, rows, Tp, segs, t.n_items,
                                         operand_dtype, st));
    // a segment of padding only has no key: the padded form skips it through seq_info, here its rows are cleared afterwards
    ESMK_TRY(launch_zero_allpad_segments(ctx_out, lse_out, tab, segs.npad, n_seg, H, rows,
                                         (size_t)H * head_dim * op_size(operand_dtype), st));
    ESMK_TRY(hipStreamSynchronize(st));  // the work list is freed on return
    return 0;
}

int esmk_op_attention_probs_packed(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                                   const int32_t* segments_host, int n_seg, int rows, int H, int head_dim, int L_total,
                                   int layer, int operand_dtype, int lowp, void* probs_out, size_t probs_elems, void* stream) {
    const std::string w("esmk_op_attention_probs_packed");
    if (!q_dev || !k_dev || !lse_dev) return fail(w + ": null argument");
    if (H <= 0 || L_total <= 0) return fail(w + ": H and L_total must be positive");
    if (head_dim != 64 && head_dim != 128) return fail(w + ": head_dim must be 64 or 128");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16) return fail(w + ": operand_dtype must be fp16 or bf16");
    if (layer < 0 || layer >= L_total) return fail(w + ": layer out of range");
    PackedOpTables t;
    if (packed_op_tables(w, segments_host, n_seg, rows, &t)) return 1;
    if (!probs_out) return fail(w + ": attention buffer missing");
    const unsigned long long need = t.sum_len2 * (unsigned long long)L_total * (unsigned long long)H;
    if ((unsigned long long)probs_elems < need)
        return fail(w + ": attention buffer too small (" + std::to_string(probs_elems) + " elements, need " + std::to_string(need) +
                    " = L H sum(len^2))");
    hipStream_t st = (hipStream_t)stream;
    DevBuf d;
    ESMK_TRY(hipMalloc(&d.p, t.host.size() * 4));
    ESMK_TRY(hipMemcpy(d.p, t.host.data(), t.host.size() * 4, hipMemcpyHostToDevice));
    int* tab = (int*)d.p;
    AttnSegs segs;
    segs.npad = tab + (size_t)2 * n_seg;
    segs.work = tab + (size_t)3 * n_seg;
    const unsigned long long* map_off = reinterpret_cast<const unsigned long long*>(tab + t.map_base);
    ESMK_TRY(launch_seg_npad(key_bias_dev, tab, n_seg, tab + (size_t)2 * n_seg, st));
    if (head_dim == 128)
        ESMK_TRY(launch_attention_probs128_packed(q_dev, k_dev, lse_dev, key_bias_dev, probs_out, H, rows, layer, L_total, segs,
                                                  map_off, t.n_items, operand_dtype, lowp != 0, st));
    else
        ESMK_TRY(launch_attention_probs_packed(q_dev, k_dev, lse_dev, key_bias_dev, probs_out, H, rows, layer, L_total, segs,
                                               map_off, t.n_items, operand_dtype, lowp != 0, st));
    ESMK_TRY(hipStreamSynchronize(st));  // the work list is freed on return
    return 0;
}

// Contact pipeline of the fused path (contacts.hip) on caller-supplied q, k and lse, stacked over layers
// (tests/test_contacts_kernels_gpu.py).  Validation and planning shared by the two entries below; the launches are
// the engine's own.  Packed form (seg != NULL): B = 1, T = rows; segments may leave gaps, start anywhere, come in any
// order and be empty, but must not overlap.  G: 0 = the engine's head-group count, else a forced one, raised to the
// count whose groups all hold a head (ceil(H / ceil(H / G))).
struct CtOpLayout {
    int G = 0;
    CtPackedPlan plan;
    size_t acc = 0, row = 0, col = 0, rowp = 0, colp = 0, wt = 0, tables = 0, total = 0;
    size_t ct_base = 0, n_int = 0;  // packed: int32 slot of the contact tables, int32 slots uploaded
};

static int contacts_op_plan(const char* who, int B, int H, int T, int L, int head_dim, const int32_t* seg, int n_seg,
                            int prepend_bos, int append_eos, int G_req, CtOpLayout* lay) {
    const std::string w(who);
    if (B <= 0 || H <= 0 || T <= 0 || L <= 0) return fail(w + ": B, H, T and num_layers must be positive");
    if (head_dim != 64 && head_dim != 128) return fail(w + ": head_dim must be 64 or 128");
    if ((prepend_bos != 0 && prepend_bos != 1) || (append_eos != 0 && append_eos != 1))
        return fail(w + ": prepend_bos and append_eos must be 0 or 1");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    if ((long long)L * H > (1 << 20)) return fail(w + ": num_layers * H is too large");
    if (G_req < 0 || G_req > H) return fail(w + ": head_groups must be 0 (engine's choice) or in [1, H]");
    if (G_req > 0 && head_dim == 128 && (H + G_req - 1) / G_req > 20)
        return fail(w + ": head_dim 128 takes at most 20 heads per group");
    const size_t C = (size_t)L * H;
    Carve c;
    if (seg == nullptr) {
        if (n_seg != 0) return fail(w + ": n_seg without a segment table");
        if (T - prepend_bos - append_eos <= 0) return fail(w + ": no contact map: T - prepend_bos - append_eos <= 0");
        const long long nQ = (T + 127) / 128;
        lay->G = contacts_head_groups((long long)B * nQ * nQ, H, head_dim);
        if (G_req > 0) {
            const int hg = (H + G_req - 1) / G_req;
            lay->G = (H + hg - 1) / hg;
        }
        lay->acc = c.take((size_t)lay->G * B * T * T * 4);
        lay->row = c.take((size_t)B * C * T * 4);
        lay->col = c.take((size_t)B * C * T * 4);
        lay->rowp = c.take((size_t)B * nQ * H * T * 4);
        lay->colp = c.take((size_t)B * ((T + 31) / 32) * H * T * 4);
        lay->wt = c.take((size_t)B * C * 4);
    } else {
        if (B != 1) return fail(w + ": the packed form takes B = 1 (T = rows)");
        if (n_seg <= 0) return fail(w + ": n_seg must be positive");
        std::vector<std::pair<long long, long long>> span;
        for (int s = 0; s < n_seg; ++s) {
            const long long start = seg[2 * s], len = seg[2 * s + 1];
            if (start < 0 || len < 0 || start + len > T)
                return fail(w + ": segment table: every segment must lie inside [0, rows)");
            if (len > 0) span.emplace_back(start, start + len);
        }
        std::sort(span.begin(), span.end());
        for (size_t i = 1; i < span.size(); ++i)
            if (span[i].first < span[i - 1].second) return fail(w + ": segment table: segments overlap");
        lay->plan = contacts_packed_plan(seg, n_seg, H, head_dim, prepend_bos, append_eos);
        if (G_req > 0) {
            const int hg = (H + G_req - 1) / G_req;
            lay->plan.G = (H + hg - 1) / hg;
        }
        lay->G = lay->plan.G;
        const CtPackedPlan& p = lay->plan;
        lay->acc = c.take((size_t)p.G * p.sum_len2 * 4);
        lay->row = c.take(C * T * 4);
        lay->col = c.take(C * T * 4);
        lay->rowp = c.take((size_t)p.rowp * 4);
        lay->colp = c.take((size_t)p.colp * 4);
        lay->wt = c.take((size_t)n_seg * C * 4);
        lay->ct_base = ((size_t)2 * n_seg + 1) & ~(size_t)1;  // [seg 2 n_seg] | contact tables (8-byte aligned)
        lay->n_int = lay->ct_base + p.table_ints();
        lay->tables = c.take(lay->n_int * 4);
    }
    lay->total = c.off;
    return 0;
}

int esmk_op_contacts_fused_workspace_bytes_ex(int B, int H, int T, int num_layers, int head_dim,
                                              const int32_t* segments_host, int n_seg, int prepend_bos, int append_eos,
                                              int head_groups, size_t* bytes) {
    if (!bytes) return fail("esmk_op_contacts_fused_workspace_bytes_ex: null argument");
    CtOpLayout lay;
    if (contacts_op_plan("esmk_op_contacts_fused_workspace_bytes_ex", B, H, T, num_layers, head_dim, segments_host,
                         n_seg, prepend_bos, append_eos, head_groups, &lay))
        return 1;
    *bytes = lay.total;
    return 0;
}

int esmk_op_contacts_fused_ex(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                              const int64_t* tokens_dev, const float* w_dev, const float* b_dev,
                              const int32_t* segments_host, int n_seg, float* out_dev, void* workspace_dev,
                              size_t workspace_bytes, int B, int H, int T, int num_layers, int head_dim, int pad_idx,
                              int eos_idx, int prepend_bos, int append_eos, int head_groups, int* head_groups_used,
                              int operand_dtype, void* stream) {
    const char* who = "esmk_op_contacts_fused_ex";
    if (!q_dev || !k_dev || !lse_dev || !tokens_dev || !w_dev || !out_dev || !workspace_dev)
        return fail("esmk_op_contacts_fused_ex: null argument");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_contacts_fused_ex: operand_dtype must be fp16 or bf16");
    CtOpLayout lay;
    if (contacts_op_plan(who, B, H, T, num_layers, head_dim, segments_host, n_seg, prepend_bos, append_eos,
                         head_groups, &lay))
        return 1;
    if (workspace_bytes < lay.total) return fail("esmk_op_contacts_fused_ex: workspace too small");
    if (head_groups_used) *head_groups_used = lay.G;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    const int L = num_layers, C = L * H;
    const size_t os = op_size(operand_dtype);
    // one layer of q / k: [B, H, T, D] padded, [H, rows, D] packed (B = 1, T = rows): the same stride
    const size_t qk_layer = (size_t)B * H * T * head_dim * os, lse_layer = (size_t)B * H * T;
    float* acc = (float*)(ws + lay.acc);
    float* row = (float*)(ws + lay.row);
    float* col = (float*)(ws + lay.col);
    float* rowp = (float*)(ws + lay.rowp);
    float* colp = (float*)(ws + lay.colp);
    float* wt = (float*)(ws + lay.wt);
    if (segments_host == nullptr) {
        for (int l = 0; l < L; ++l)
            ESMK_TRY(launch_contacts_fused_layer((const char*)q_dev + l * qk_layer, (const char*)k_dev + l * qk_layer,
                                                 lse_dev + l * lse_layer, key_bias_dev, tokens_dev, w_dev, acc, row,
                                                 col, rowp, colp, B, H, T, C, l, head_dim, pad_idx, eos_idx,
                                                 prepend_bos, append_eos, operand_dtype, st, lay.G));
        ESMK_TRY(launch_contacts_fused_final(acc, row, col, wt, tokens_dev, w_dev, b_dev, out_dev, B, H, C, T, head_dim,
                                             pad_idx, eos_idx, prepend_bos, append_eos, st, lay.G));
        return 0;
    }
    // the segment table and the contact tables, uploaded as esmk_forward_packed_ex does (tables behind the workspace)
    std::vector<int32_t> host(lay.n_int, 0);
    memcpy(host.data(), segments_host, (size_t)2 * n_seg * 4);
    contacts_packed_tables(lay.plan, segments_host, prepend_bos, append_eos, H, host.data() + lay.ct_base);
    int* tab = (int*)(ws + lay.tables);
    ESMK_TRY(hipMemcpyAsync(tab, host.data(), lay.n_int * 4, hipMemcpyHostToDevice, st));
    ESMK_TRY(hipStreamSynchronize(st));  // `host` goes out of scope below
    const CtPackedPlan& p = lay.plan;
    CtPackedDev d;
    d.seg = tab;
    d.off = reinterpret_cast<const long long*>(tab + lay.ct_base);
    d.acc_work = tab + lay.ct_base + 8 * (size_t)n_seg;
    d.red_work = d.acc_work + 4 * p.n_acc;
    d.rt_work = d.red_work + 2 * p.n_red;
    d.fin_work = d.rt_work + p.n_rt;
    d.rows = T;
    for (int l = 0; l < L; ++l)
        ESMK_TRY(launch_contacts_packed_layer((const char*)q_dev + l * qk_layer, (const char*)k_dev + l * qk_layer,
                                              lse_dev + l * lse_layer, key_bias_dev, tokens_dev, w_dev, acc, row, col,
                                              rowp, colp, p, d, H, C, l, head_dim, pad_idx, eos_idx, prepend_bos,
                                              append_eos, operand_dtype, st));
    ESMK_TRY(launch_contacts_packed_final(acc, row, col, wt, tokens_dev, w_dev, b_dev, out_dev, p, d, C, pad_idx,
                                          eos_idx, prepend_bos, append_eos, st));
    return 0;
}

// The generalised-addressing GEMM forms esmk_forward / esmk_msa_forward launch, one launch at a time
// (tests/test_gemm_forms_gpu.py).  Validation only, then launch_gemm unchanged.
int esmk_op_gemm_ex(const esmk_gemm_ex_args* a, void* stream) {
    if (!a) return fail("esmk_op_gemm_ex: null argument");
    if (a->size != sizeof(esmk_gemm_ex_args)) return fail("esmk_op_gemm_ex: size must be sizeof(esmk_gemm_ex_args)");
    const int epi = a->epilogue;
    if (epi < EPI_STORE_T || epi > EPI_MSA_CTX) return fail("esmk_op_gemm_ex: epilogue must be 0 ... 7");
    if (a->operand_dtype != ESMK_DT_F16 && a->operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_gemm_ex: operand_dtype must be fp16 or bf16");
    const bool qk = epi == EPI_QKV_ROPE, vt = epi == EPI_V_T, ctx = epi == EPI_MSA_CTX;
    if (!a->A || !a->W) return fail("esmk_op_gemm_ex: null operand");
    if (qk && (!a->q || !a->k || !a->cos || !a->sin)) return fail("esmk_op_gemm_ex: epilogue 5 needs q, k, cos and sin");
    if (vt && !a->vt) return fail("esmk_op_gemm_ex: epilogue 6 needs vt");
    if (!qk && !vt && !a->out) return fail("esmk_op_gemm_ex: null output");
    if (a->M <= 0 || a->N <= 0 || a->K <= 0) return fail("esmk_op_gemm_ex: M, N and K must be positive");
    if (a->K % 64 != 0 || a->N % 8 != 0) return fail("esmk_op_gemm_ex: need K % 64 == 0 and N % 8 == 0");
    if ((qk || vt || ctx) && a->N % 64 != 0) return fail("esmk_op_gemm_ex: epilogues 5, 6 and 7 need N % 64 == 0");
    if (a->head_dim != 64 && a->head_dim != 128) return fail("esmk_op_gemm_ex: head_dim must be 64 or 128");
    if (a->head_dim == 128 && !qk && !vt) return fail("esmk_op_gemm_ex: head_dim 128 belongs to epilogues 5 and 6");
    if (a->batch < 1 || a->batch_inner < 1 || a->batch % a->batch_inner != 0)
        return fail("esmk_op_gemm_ex: batch and batch_inner must be >= 1 and batch_inner must divide batch");
    if (a->a_row_bytes < 0 || a->w_row_bytes < 0 || a->a_kt_bytes < 0 || a->w_kt_bytes < 0 || a->a_bo < 0 ||
        a->a_bi < 0 || a->w_bo < 0 || a->w_bi < 0 || a->o_bo < 0 || a->o_bi < 0 || a->n_valid < 0 || a->ldc < 0 ||
        a->vt_rows < 0 || a->rowmap_R < 0 || a->rowmap_C < 0 || a->ctx_R < 0 || a->ctx_C < 0)
        return fail("esmk_op_gemm_ex: strides, offsets and counts must not be negative");
    if (a->a_kt_repeat != 0 && (a->a_kt_repeat != 1 || a->K % 128 != 0))
        return fail("esmk_op_gemm_ex: a_kt_repeat is 0 or 1, and 1 needs K % 128 == 0");
    if (a->n_valid > a->N) return fail("esmk_op_gemm_ex: n_valid must be <= N");
    if (a->ldc > 0 && !ctx && a->ldc < a->N) return fail("esmk_op_gemm_ex: ldc must be >= N");
    if ((a->row_keep || a->row_pos) && !qk) return fail("esmk_op_gemm_ex: row_keep and row_pos belong to epilogue 5");
    if (a->vt_rows > 0 && !vt) return fail("esmk_op_gemm_ex: vt_rows belongs to epilogue 6");
    if (a->vt_rows > 0 && a->head_dim == 128) return fail("esmk_op_gemm_ex: vt_rows needs head_dim 64");
    if (qk || vt) {
        if (a->T <= 0 || a->H <= 0 || a->E != a->H * a->head_dim || a->N != (qk ? 2 : 1) * a->E || a->M % a->T != 0)
            return fail("esmk_op_gemm_ex: epilogues 5 and 6 need T, H > 0, E = H head_dim, N = 2E (5) or E (6), M % T == 0");
        if (vt && (a->Tp < a->T || a->Tp % 64 != 0)) return fail("esmk_op_gemm_ex: Tp must be a multiple of 64 and >= T");
        if (a->vt_rows > 0 && (a->M / a->T) % a->vt_rows != 0)
            return fail("esmk_op_gemm_ex: vt_rows must divide the number of sequences M / T");
    }
    if ((a->rowmap_R > 0 || a->rowmap_C > 0) &&
        (epi != EPI_RESID_F32 || a->rowmap_R <= 0 || a->rowmap_C <= 0 || a->M % (a->rowmap_R * a->rowmap_C) != 0))
        return fail("esmk_op_gemm_ex: the row map needs epilogue 4, rowmap_R, rowmap_C > 0 and M % (R C) == 0");
    if ((a->ctx_R > 0 || a->ctx_C > 0) && !ctx) return fail("esmk_op_gemm_ex: ctx_R and ctx_C belong to epilogue 7");
    if (ctx && (a->ctx_R <= 0 || a->ctx_C < a->M || a->N != 64 * a->ctx_R || a->ldc < 64 * a->batch_inner))
        return fail("esmk_op_gemm_ex: epilogue 7 needs N = 64 ctx_R, ctx_C >= M and ldc >= 64 batch_inner");
    GemmArgs g;
    g.A = a->A;
    g.W = a->W;
    g.bias = a->bias;
    g.out = a->out;
    g.M = a->M;
    g.N = a->N;
    g.K = a->K;
    g.q = a->q;
    g.k = a->k;
    g.vt = a->vt;
    g.cos = a->cos;
    g.sin = a->sin;
    g.T = a->T;
    g.H = a->H;
    g.E = a->E;
    g.Tp = a->Tp;
    g.scaling = a->scaling;
    g.a_row_bytes = a->a_row_bytes;
    g.w_row_bytes = a->w_row_bytes;
    g.a_kt_bytes = a->a_kt_bytes;
    g.w_kt_bytes = a->w_kt_bytes;
    g.a_kt_repeat = a->a_kt_repeat;
    g.batch = a->batch;
    g.batch_inner = a->batch_inner;
    g.a_bo = a->a_bo;
    g.a_bi = a->a_bi;
    g.w_bo = a->w_bo;
    g.w_bi = a->w_bi;
    g.o_bo = a->o_bo;
    g.o_bi = a->o_bi;
    g.n_valid = a->n_valid;
    g.ldc = a->ldc;
    g.row_keep = a->row_keep;
    g.vt_rows = a->vt_rows;
    g.rowmap_R = a->rowmap_R;
    g.rowmap_C = a->rowmap_C;
    g.ctx_R = a->ctx_R;
    g.ctx_C = a->ctx_C;
    g.head_dim = a->head_dim;
    g.row_pos = a->row_pos;
    if (epi == EPI_GELU_F32 && gemm8_generalised(g, epi))
        return fail("esmk_op_gemm_ex: epilogue 3 (fp32 gelu) has no generalised form");
    ESMK_TRY(launch_gemm(g, epi, a->operand_dtype, (hipStream_t)stream));
    return 0;
}

int esmk_op_msa_row_softmax(const float* scores_dev, const float* keep_dev, const int32_t* any_pad_dev, void* probs_out,
                            float* attn_out, int B, int H, int R, int C, int ldp, int layer, int num_layers_total,
                            int nslice, int operand_dtype, void* stream) {
    if (!scores_dev || !keep_dev || !any_pad_dev || !probs_out) return fail("esmk_op_msa_row_softmax: null argument");
    if (B <= 0 || H <= 0 || R <= 0 || C <= 0) return fail("esmk_op_msa_row_softmax: B, H, R and C must be positive");
    if (C > 1024 || ldp > 1024 || ldp < C) return fail("esmk_op_msa_row_softmax: need C <= ldp <= 1024");
    if (nslice < 1) return fail("esmk_op_msa_row_softmax: nslice must be >= 1");
    if (attn_out && (layer < 0 || layer >= num_layers_total)) return fail("esmk_op_msa_row_softmax: layer out of range");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16)
        return fail("esmk_op_msa_row_softmax: operand_dtype must be fp16 or bf16");
    ESMK_TRY(launch_msa_row_softmax(scores_dev, keep_dev, any_pad_dev, probs_out, attn_out, B, H, R, C, ldp, layer,
                                    num_layers_total, operand_dtype, (hipStream_t)stream, nslice));
    return 0;
}

int esmk_op_mask_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_dev, int64_t* out_dev, int B,
                      int T, int n, int mask_idx, void* stream) {
    if (!tokens_dev || !pos_dev || !out_dev) return fail("esmk_op_mask_rows: null argument");
    if (B <= 0 || T <= 0 || n <= 0) return fail("esmk_op_mask_rows: B, T and n must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS || (long long)n * T > ESMK_MAX_ROWS)
        return fail("esmk_op_mask_rows: B*T or n*T exceeds 2^24 rows");
    ESMK_TRY(launch_copy_rows(tokens_dev, src_row_dev, /*start=*/nullptr, /*pos_off=*/nullptr, pos_dev, /*tok=*/nullptr, out_dev, B, T,
                              n, T, /*total=*/0, /*V=*/0, /*head_tok=*/-1, /*tail_tok=*/-1, mask_idx, (hipStream_t)stream));
    return 0;
}

int esmk_op_mask_rows_multi(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_off_dev,
                            const int32_t* pos_dev, int64_t* out_dev, int B, int T, int n, int total, int mask_idx, void* stream) {
    if (!tokens_dev || !pos_off_dev || !pos_dev || !out_dev) return fail("esmk_op_mask_rows_multi: null argument");
    if (B <= 0 || T <= 0 || n <= 0) return fail("esmk_op_mask_rows_multi: B, T and n must be positive");
    if (total < 0) return fail("esmk_op_mask_rows_multi: total must not be negative");
    if ((long long)B * T > ESMK_MAX_ROWS || (long long)n * T > ESMK_MAX_ROWS)
        return fail("esmk_op_mask_rows_multi: B*T or n*T exceeds 2^24 rows");
    ESMK_TRY(launch_copy_rows(tokens_dev, src_row_dev, /*start=*/nullptr, pos_off_dev, pos_dev, /*tok=*/nullptr, out_dev, B, T, n, T,
                              total, /*V=*/0, /*head_tok=*/-1, /*tail_tok=*/-1, mask_idx, (hipStream_t)stream));
    return 0;
}

int esmk_op_score_rows(const float* logprobs_dev, const int32_t* wt_dev, const int32_t* mt_dev, const int32_t* var_off_dev,
                       double* out_dev, int n_rows, int n_var, int V, void* stream) {
    if (!logprobs_dev || !wt_dev || !mt_dev || !var_off_dev || !out_dev) return fail("esmk_op_score_rows: null argument");
    if (n_rows <= 0 || n_var <= 0 || V <= 0) return fail("esmk_op_score_rows: n_rows, n_var and V must be positive");
    ESMK_TRY(launch_score_rows(logprobs_dev, wt_dev, mt_dev, var_off_dev, out_dev, n_rows, n_var, V, (hipStream_t)stream));
    return 0;
}

int esmk_op_mask_rows_packed(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* seg_start_dev,
                             const int32_t* seg_len_dev, const int32_t* pos_off_dev, const int32_t* pos_dev, int64_t* out_dev, int B,
                             int T, int n, int total, int rows, int mask_idx, int pad_idx, void* stream) {
    if (!tokens_dev || !src_row_dev || !seg_start_dev || !seg_len_dev || !pos_off_dev || !pos_dev || !out_dev)
        return fail("esmk_op_mask_rows_packed: null argument");
    if (B <= 0 || T <= 0 || n <= 0) return fail("esmk_op_mask_rows_packed: B, T and n must be positive");
    if (total < 0) return fail("esmk_op_mask_rows_packed: total must not be negative");
    if (rows <= 0 || rows % 64 != 0 || rows > ESMK_MAX_ROWS)
        return fail("esmk_op_mask_rows_packed: need 0 < rows <= 2^24, rows % 64 == 0");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail("esmk_op_mask_rows_packed: B*T exceeds 2^24 rows");
    ESMK_TRY(launch_mask_rows_packed(tokens_dev, src_row_dev, seg_start_dev, seg_len_dev, pos_off_dev, pos_dev, out_dev, B, T, n,
                                     total, rows, mask_idx, pad_idx, (hipStream_t)stream));
    return 0;
}

int esmk_op_sum_target_rows(const float* logprobs_dev, const int32_t* target_dev, const int32_t* off_dev, double* out_dev,
                            int n_rows, int n_seq, int V, void* stream) {
    if (!logprobs_dev || !target_dev || !off_dev || !out_dev) return fail("esmk_op_sum_target_rows: null argument");
    if (n_rows <= 0 || n_seq <= 0 || V <= 0) return fail("esmk_op_sum_target_rows: n_rows, n_seq and V must be positive");
    ESMK_TRY(launch_sum_target_rows(logprobs_dev, target_dev, off_dev, out_dev, n_rows, n_seq, V, (hipStream_t)stream));
    return 0;
}

int esmk_op_window_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* start_dev,
                        const int32_t* mask_off_dev, const int32_t* mask_pos_dev, int64_t* out_dev, int B, int T, int n, int Tw,
                        int total, int head_tok, int tail_tok, int mask_idx, void* stream) {
    if (!tokens_dev || !src_row_dev || !start_dev || !mask_off_dev || !mask_pos_dev || !out_dev)
        return fail("esmk_op_window_rows: null argument");
    if (B <= 0 || T <= 0 || n <= 0 || Tw <= 0) return fail("esmk_op_window_rows: B, T, n and Tw must be positive");
    if (total < 0) return fail("esmk_op_window_rows: total must not be negative");
    if ((long long)B * T > ESMK_MAX_ROWS || (long long)n * Tw > ESMK_MAX_ROWS)
        return fail("esmk_op_window_rows: B*T or n*Tw exceeds 2^24 rows");
    ESMK_TRY(launch_copy_rows(tokens_dev, src_row_dev, start_dev, mask_off_dev, mask_pos_dev, /*tok=*/nullptr, out_dev, B, T, n, Tw,
                              total, /*V=*/0, head_tok, tail_tok, mask_idx, (hipStream_t)stream));
    return 0;
}

int esmk_op_blend_rows(const void* x_dev, int x_dtype, const int32_t* off_dev, const int32_t* src_dev, const float* w_dev,
                       float* out_dev, int N, int E, int n_out, int total, void* stream) {
    if (!x_dev || !off_dev || !src_dev || !w_dev || !out_dev) return fail("esmk_op_blend_rows: null argument");
    if (N <= 0 || n_out <= 0) return fail("esmk_op_blend_rows: N and n_out must be positive");
    if (E <= 0 || E % 4 != 0) return fail("esmk_op_blend_rows: E must be a positive multiple of 4");
    if (total < 0) return fail("esmk_op_blend_rows: total must not be negative");
    if (x_dtype != ESMK_DT_F32 && x_dtype != ESMK_DT_F16 && x_dtype != ESMK_DT_BF16)
        return fail("esmk_op_blend_rows: x_dtype must be ESMK_F32, ESMK_F16 or ESMK_BF16");
    ESMK_TRY(launch_blend_rows(x_dev, x_dtype, off_dev, src_dev, w_dev, out_dev, N, E, n_out, total, (hipStream_t)stream));
    return 0;
}

int esmk_op_stitch_contacts(const float* maps_dev, const int32_t* start_dev, float* out_dev, int n_w, int R, int Lb, int body_lo,
                            void* stream) {
    if (!maps_dev || !start_dev || !out_dev) return fail("esmk_op_stitch_contacts: null argument");
    if (n_w <= 0 || R <= 0 || Lb <= 0) return fail("esmk_op_stitch_contacts: n_w, R and Lb must be positive");
    if ((long long)n_w * R * R > (1ll << 40) || Lb > (1 << 20))
        return fail("esmk_op_stitch_contacts: n_w*R*R exceeds 2^40 entries or Lb exceeds 2^20");
    ESMK_TRY(launch_stitch_contacts(maps_dev, start_dev, out_dev, n_w, R, Lb, body_lo, (hipStream_t)stream));
    return 0;
}

int esmk_op_log_softmax_rows(const float* logits_dev, float* out_dev, const int32_t* target_dev, float* target_out_dev, int n,
                             int V, void* stream) {
    if (!logits_dev || !out_dev) return fail("esmk_op_log_softmax_rows: null argument");
    if ((target_dev != nullptr) != (target_out_dev != nullptr))
        return fail("esmk_op_log_softmax_rows: target_dev and target_out_dev go together");
    if (n <= 0 || n > ESMK_MAX_ROWS) return fail("esmk_op_log_softmax_rows: n must be in 1 .. 2^24");
    if (V <= 0 || V > 64) return fail("esmk_op_log_softmax_rows: V must be in 1 .. 64 (one vocabulary entry per lane)");
    ESMK_TRY(launch_log_softmax_rows(logits_dev, out_dev, target_dev, target_out_dev, n, V, (hipStream_t)stream));
    return 0;
}

// ---- sampling (sampling.hip; esm_amd/sampling.py) ---------------------------------------------------------------------
int esmk_op_permute_positions(const int32_t* pos_off_dev, const int32_t* pos_in_dev, const int32_t* chain_id_dev,
                              int32_t* perm_out_dev, int n_chain, int total, uint64_t seed, int epoch, void* stream) {
    if (!pos_off_dev || !pos_in_dev || !chain_id_dev || !perm_out_dev) return fail("esmk_op_permute_positions: null argument");
    if (n_chain <= 0 || total <= 0) return fail("esmk_op_permute_positions: n_chain and total must be positive");
    if (epoch < 0) return fail("esmk_op_permute_positions: epoch must not be negative");
    ESMK_TRY(launch_permute_positions(pos_off_dev, pos_in_dev, chain_id_dev, perm_out_dev, n_chain, total,
                                      (unsigned long long)seed, epoch, (hipStream_t)stream));
    return 0;
}

// what esmk_op_sample_rows and esmk_op_sample_rows_ex refuse alike, under the entry's own name
static int sample_rows_check(const std::string& w, const void* lp, const void* row_chain, const void* row_index, const void* token_out,
                             const void* logq_out, int n, int V, float inv_temperature, int step) {
    if (!lp || !row_chain || !row_index || !token_out || !logq_out) return fail(w + ": null argument");
    if (n <= 0 || n > ESMK_MAX_ROWS) return fail(w + ": n must be in 1 .. 2^24");
    if (V <= 0 || V > 64) return fail(w + ": V must be in 1 .. 64 (one vocabulary entry per lane)");
    if (!(inv_temperature >= 0.f) || inv_temperature > 3.0e38f)
        return fail(w + ": inv_temperature must be finite and not negative (0: greedy)");
    if (step < 0) return fail(w + ": step must not be negative");
    return 0;
}

int esmk_op_sample_rows(const float* logprobs_dev, const int32_t* row_chain_dev, const int32_t* row_index_dev,
                        const int32_t* exclude_dev, uint64_t allowed_mask, float inv_temperature, uint64_t seed, int step,
                        int32_t* token_out_dev, float* logq_out_dev, float* u_out_dev, int n, int V, void* stream) {
    if (int rc = sample_rows_check("esmk_op_sample_rows", logprobs_dev, row_chain_dev, row_index_dev, token_out_dev, logq_out_dev, n,
                                   V, inv_temperature, step))
        return rc;
    ESMK_TRY(launch_sample_rows(logprobs_dev, row_chain_dev, row_index_dev, exclude_dev, (unsigned long long)allowed_mask,
                                inv_temperature, (unsigned long long)seed, step, /*top_k=*/0, /*top_p=*/1.f, /*score_kind=*/0,
                                token_out_dev, logq_out_dev, u_out_dev, /*score_out=*/nullptr, /*kept_out=*/nullptr, n, V,
                                (hipStream_t)stream));
    return 0;
}

int esmk_op_sample_rows_ex(const float* logprobs_dev, const int32_t* row_chain_dev, const int32_t* row_index_dev,
                           const int32_t* exclude_dev, uint64_t allowed_mask, float inv_temperature, uint64_t seed, int step,
                           int top_k, float top_p, int score_kind, int32_t* token_out_dev, float* logq_out_dev, float* u_out_dev,
                           float* score_out_dev, uint64_t* kept_out_dev, int n, int V, void* stream) {
    if (int rc = sample_rows_check("esmk_op_sample_rows_ex", logprobs_dev, row_chain_dev, row_index_dev, token_out_dev, logq_out_dev,
                                   n, V, inv_temperature, step))
        return rc;
    if (top_k < 0 || top_k > 64) return fail("esmk_op_sample_rows_ex: top_k must be in 0 .. 64 (0: off)");
    if (!(top_p > 0.f && top_p <= 1.f)) return fail("esmk_op_sample_rows_ex: top_p must be in (0, 1] (1: off)");
    if (score_kind < 0 || score_kind > 2)
        return fail("esmk_op_sample_rows_ex: score_kind must be 0 (none), 1 (confidence) or 2 (negative entropy)");
    if (score_kind != 0 && !score_out_dev) return fail("esmk_op_sample_rows_ex: a score_kind other than 0 needs score_out_dev");
    ESMK_TRY(launch_sample_rows(logprobs_dev, row_chain_dev, row_index_dev, exclude_dev, (unsigned long long)allowed_mask,
                                inv_temperature, (unsigned long long)seed, step, top_k, top_p, score_kind, token_out_dev,
                                logq_out_dev, u_out_dev, score_out_dev, (unsigned long long*)kept_out_dev, n, V,
                                (hipStream_t)stream));
    return 0;
}

int esmk_op_select_rows(const float* score_dev, const int32_t* row_off_dev, const int32_t* sel_off_dev,
                        const int32_t* rest_off_dev, int32_t* sel_out_dev, int32_t* rest_out_dev, int n_chain, int n, int n_sel,
                        int n_rest, void* stream) {
    if (!score_dev || !row_off_dev || !sel_off_dev || !sel_out_dev) return fail("esmk_op_select_rows: null argument");
    if (n_chain <= 0 || n_chain > ESMK_MAX_ROWS || n <= 0 || n > ESMK_MAX_ROWS || n_sel <= 0 || n_sel > ESMK_MAX_ROWS)
        return fail("esmk_op_select_rows: n_chain, n and n_sel must be in 1 .. 2^24");
    if (n_rest < 0 || n_rest > ESMK_MAX_ROWS) return fail("esmk_op_select_rows: n_rest must be in 0 .. 2^24");
    if (n_rest > 0 && (!rest_off_dev || !rest_out_dev))
        return fail("esmk_op_select_rows: n_rest > 0 needs rest_off_dev and rest_out_dev");
    ESMK_TRY(launch_select_rows(score_dev, row_off_dev, sel_off_dev, rest_off_dev, sel_out_dev, rest_out_dev, n_chain, n, n_sel,
                                n_rest, (hipStream_t)stream));
    return 0;
}

int esmk_op_commit_tokens(int64_t* tokens_dev, const int32_t* row_chain_slot_dev, const int32_t* pos_dev,
                          const int32_t* token_dev, int n, int B, int T, void* stream) {
    if (!tokens_dev || !row_chain_slot_dev || !pos_dev || !token_dev) return fail("esmk_op_commit_tokens: null argument");
    if (n <= 0 || B <= 0 || T <= 0) return fail("esmk_op_commit_tokens: n, B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS || n > ESMK_MAX_ROWS) return fail("esmk_op_commit_tokens: B*T or n exceeds 2^24 rows");
    ESMK_TRY(launch_commit_tokens(tokens_dev, row_chain_slot_dev, pos_dev, token_dev, n, B, T, (hipStream_t)stream));
    return 0;
}

// ---- Metropolis-Hastings design (design.hip): everything is refused here before any HIP call ---------------------------
int esmk_op_propose_mutations(const int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* pos_off_dev, const int32_t* pos_dev,
                              const int32_t* chain_id_dev, uint64_t allowed_mask, int force_new, uint64_t seed, int step,
                              int32_t* site_out_dev, int32_t* old_out_dev, int32_t* tok_out_dev, int n_chain, int B, int T, int total,
                              int V, void* stream) {
    if (!tokens_dev || !pos_off_dev || !pos_dev || !chain_id_dev || !site_out_dev || !old_out_dev || !tok_out_dev)
        return fail("esmk_op_propose_mutations: null argument");
    if (n_chain <= 0 || B <= 0 || T <= 0) return fail("esmk_op_propose_mutations: n_chain, B and T must be positive");
    if (total < 0) return fail("esmk_op_propose_mutations: total must not be negative");
    if ((long long)B * T > ESMK_MAX_ROWS || n_chain > ESMK_MAX_ROWS) return fail("esmk_op_propose_mutations: B*T or n_chain exceeds 2^24 rows");
    if (V <= 0 || V > 64) return fail("esmk_op_propose_mutations: V must be in 1 .. 64 (the candidate set is a 64-bit mask)");
    if (step < 0) return fail("esmk_op_propose_mutations: step must not be negative");
    ESMK_TRY(launch_propose_mutations(tokens_dev, slot_dev, pos_off_dev, pos_dev, chain_id_dev, (unsigned long long)allowed_mask,
                                      force_new ? 1 : 0, (unsigned long long)seed, step, site_out_dev, old_out_dev, tok_out_dev,
                                      n_chain, B, T, total, V, (hipStream_t)stream));
    return 0;
}

int esmk_op_contact_energy(const float* contacts_dev, const uint8_t* target_dev, double* energy_out_dev, int32_t* count_out_dev, int B,
                           int S, int min_sep, int kind, void* stream) {
    if (!contacts_dev || !target_dev || !energy_out_dev || !count_out_dev) return fail("esmk_op_contact_energy: null argument");
    if (B <= 0 || S <= 0) return fail("esmk_op_contact_energy: B and S must be positive");
    if (S > 32768) return fail("esmk_op_contact_energy: S above 32768 (the pairs of a map are indexed in 32 bits)");
    if (B > ESMK_MAX_ROWS) return fail("esmk_op_contact_energy: B exceeds 2^24");
    if (min_sep < 1) return fail("esmk_op_contact_energy: min_sep must be at least 1");
    if (kind < 0 || kind > 1) return fail("esmk_op_contact_energy: kind must be 0 (pos) or 1 (bce)");
    ESMK_TRY(launch_contact_energy(contacts_dev, target_dev, energy_out_dev, count_out_dev, B, S, min_sep, kind, (hipStream_t)stream));
    return 0;
}

// ---- linear pairwise heads on the attention maps (pair_head.hip) ---------------------------------------------------
static int pair_head_op_check(const std::string& w, int B, int H, int T, int L, int head_dim, int n_sym, int n_asym,
                              int prepend_bos, int append_eos) {
    if (B <= 0 || H <= 0 || T <= 0 || L <= 0) return fail(w + ": B, H, T and num_layers must be positive");
    if (head_dim != 64 && head_dim != 128) return fail(w + ": head_dim must be 64 or 128");
    if ((prepend_bos != 0 && prepend_bos != 1) || (append_eos != 0 && append_eos != 1))
        return fail(w + ": prepend_bos and append_eos must be 0 or 1");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    if ((long long)L * H > (1 << 20)) return fail(w + ": num_layers * H is too large");
    if (n_sym < 0 || n_asym < 0 || n_sym + n_asym <= 0 || n_sym + n_asym > 64)
        return fail(w + ": n_sym and n_asym must not be negative, n_sym + n_asym must be 1 .. 64");
    if (T - prepend_bos - append_eos <= 0) return fail(w + ": no pair map: T - prepend_bos - append_eos <= 0");
    return 0;
}

int esmk_op_pair_head_workspace_bytes(int H, int num_layers, size_t* bytes) {
    if (!bytes) return fail("esmk_op_pair_head_workspace_bytes: null argument");
    if (H <= 0 || num_layers <= 0 || (long long)num_layers * H > (1 << 20))
        return fail("esmk_op_pair_head_workspace_bytes: H and num_layers must be positive, num_layers * H at most 2^20");
    *bytes = (size_t)num_layers * H * 64 * 4;
    return 0;
}

int esmk_op_pair_head(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                      const int64_t* tokens_dev, const float* w_dev, const float* bias_dev, int n_sym, int n_asym, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, int B, int H, int T, int num_layers, int head_dim, int pad_idx,
                      int prepend_bos, int append_eos, int operand_dtype, void* stream) {
    const std::string who("esmk_op_pair_head");
    if (!q_dev || !k_dev || !lse_dev || !w_dev || !out_dev || !workspace_dev) return fail(who + ": null argument");
    if (operand_dtype != ESMK_DT_F16 && operand_dtype != ESMK_DT_BF16) return fail(who + ": operand_dtype must be fp16 or bf16");
    if (pair_head_op_check(who, B, H, T, num_layers, head_dim, n_sym, n_asym, prepend_bos, append_eos)) return 1;
    const int C = num_layers * H, C_out = n_sym + n_asym;
    if (workspace_bytes < (size_t)C * 64 * 4) return fail(who + ": workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* w64 = (float*)workspace_dev;
    ESMK_TRY(launch_pair_head_pad_w(w_dev, w64, C, C_out, st));
    ESMK_TRY(launch_pair_head(q_dev, k_dev, lse_dev, key_bias_dev, tokens_dev, w64, bias_dev, out_dev, num_layers, B, H, T, head_dim,
                              n_sym, n_asym, pad_idx, prepend_bos, append_eos, operand_dtype, st));
    return 0;
}

int esmk_op_distogram_energy(const float* pair_logits_dev, int ld, int first, int n_bins, const uint8_t* target_bin_dev, int B, int S,
                             int min_sep, double inv_temp, double* energy_out_dev, int32_t* count_out_dev, void* stream) {
    const std::string who("esmk_op_distogram_energy");
    if (!pair_logits_dev || !target_bin_dev || !energy_out_dev || !count_out_dev) return fail(who + ": null argument");
    if (B <= 0 || S <= 0) return fail(who + ": B and S must be positive");
    if (S > 32768) return fail(who + ": S above 32768 (the pairs of a map are indexed in 32 bits)");
    if (B > ESMK_MAX_ROWS) return fail(who + ": B exceeds 2^24");
    if (n_bins <= 0 || n_bins > 255) return fail(who + ": n_bins must be 1 .. 255 (255 is the ignore label)");
    if (first < 0 || ld <= 0 || first + n_bins > ld) return fail(who + ": the bins first .. first + n_bins must lie inside the ld outputs of a pair");
    if (min_sep < 0) return fail(who + ": min_sep must not be negative");
    if (!(inv_temp > 0.0) || !std::isfinite(inv_temp)) return fail(who + ": inv_temp must be positive and finite");
    ESMK_TRY(launch_distogram_energy(pair_logits_dev, ld, first, n_bins, target_bin_dev, energy_out_dev, count_out_dev, B, S, min_sep,
                                     inv_temp, (hipStream_t)stream));
    return 0;
}

// what esmk_op_mh_accept and esmk_op_mh_accept_ex refuse alike, under the entry's own name; the temperature (a scalar there, a
// table here) and the weights are the entry's own
static int mh_accept_check(const std::string& w, bool null_arg, const void* lp_sum, const void* n_res, int n_chain, int B, int T) {
    if (null_arg) return fail(w + ": null argument");
    if (lp_sum && !n_res) return fail(w + ": lp_sum without n_res");
    if (n_chain <= 0 || B <= 0 || T <= 0) return fail(w + ": n_chain, B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS || n_chain > ESMK_MAX_ROWS) return fail(w + ": B*T or n_chain exceeds 2^24 rows");
    return 0;
}

int esmk_op_mh_accept(int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* site_dev, const int32_t* tok_dev,
                      const int32_t* chain_id_dev, const double* e_contact_dev, const double* lp_sum_dev, const int32_t* n_res_dev,
                      const double* hastings_dev, double w_contact, double w_lm, double inv_temperature, uint64_t seed, int step,
                      double* e_cur_dev, double* e_contact_cur_dev, double* e_lm_cur_dev, uint8_t* accepted_out_dev, double* u_out_dev,
                      double* e_prop_out_dev, int n_chain, int B, int T, void* stream) {
    if (int rc = mh_accept_check("esmk_op_mh_accept",
                                 !tokens_dev || !site_dev || !tok_dev || !chain_id_dev || !e_cur_dev || !accepted_out_dev, lp_sum_dev,
                                 n_res_dev, n_chain, B, T))
        return rc;
    if (!(inv_temperature >= 0.0)) return fail("esmk_op_mh_accept: inv_temperature must not be negative or NaN (+inf: greedy)");
    if (!std::isfinite(w_contact) || !std::isfinite(w_lm)) return fail("esmk_op_mh_accept: the weights must be finite");
    if (step < 0) return fail("esmk_op_mh_accept: step must not be negative");
    ESMK_TRY(launch_mh_accept(tokens_dev, slot_dev, site_dev, tok_dev, chain_id_dev, e_contact_dev, lp_sum_dev, n_res_dev, hastings_dev,
                              /*e_extra=*/nullptr, w_contact, w_lm, /*w_extra=*/0.0, /*inv_t_tab=*/nullptr, inv_temperature,
                              /*rung=*/nullptr, /*n_rung=*/0, (unsigned long long)seed, step, e_cur_dev, e_contact_cur_dev,
                              e_lm_cur_dev, /*e_extra_cur=*/nullptr, accepted_out_dev, u_out_dev, e_prop_out_dev, n_chain, B, T,
                              (hipStream_t)stream));
    return 0;
}

int esmk_op_hastings_rows(const float* logprobs_dev, const int32_t* old_dev, const int32_t* new_dev, float inv_t_prop,
                          double* h_out_dev, int n, int V, void* stream) {
    if (!logprobs_dev || !old_dev || !new_dev || !h_out_dev) return fail("esmk_op_hastings_rows: null argument");
    if (n <= 0 || n > ESMK_MAX_ROWS) return fail("esmk_op_hastings_rows: n must be in 1 .. 2^24");
    if (V <= 0 || V > 64) return fail("esmk_op_hastings_rows: V must be in 1 .. 64");
    if (!(inv_t_prop >= 0.f) || inv_t_prop > 3.0e38f) return fail("esmk_op_hastings_rows: inv_t_prop must be finite and not negative");
    ESMK_TRY(launch_hastings_rows(logprobs_dev, old_dev, new_dev, inv_t_prop, h_out_dev, n, V, (hipStream_t)stream));
    return 0;
}

// ---- the n-gram term and replica exchange (tempering.hip): everything is refused here before any HIP call ---------------
int esmk_op_ngram_energy(const int64_t* tokens_dev, const int32_t* code_dev, const double* q1_dev, const double* q2_dev,
                         const double* q3_dev, const double* q4_dev, int order_mask, double* energy_out_dev, int B, int T, int first,
                         int S, int V, int A, void* stream) {
    if (!tokens_dev || !code_dev || !energy_out_dev) return fail("esmk_op_ngram_energy: null argument");
    if (B <= 0 || T <= 0) return fail("esmk_op_ngram_energy: B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail("esmk_op_ngram_energy: B*T exceeds 2^24 rows");
    if (S <= 0) return fail("esmk_op_ngram_energy: S must be positive");
    if (S > 32768) return fail("esmk_op_ngram_energy: S above 32768 (the codes of a chain are staged in 32 KiB of LDS)");
    if (first < 0 || (long long)first + S > T) return fail("esmk_op_ngram_energy: the residues first .. first + S - 1 must lie in [0, T)");
    if (V <= 0 || V > 64) return fail("esmk_op_ngram_energy: V must be in 1 .. 64");
    if (A <= 0 || A > 32) return fail("esmk_op_ngram_energy: A must be in 1 .. 32");
    if ((order_mask & 15) == 0 || (order_mask & ~15) != 0)
        return fail("esmk_op_ngram_energy: order_mask must choose at least one of the orders 1 .. 4 (bits 0 .. 3) and nothing else");
    const NgramTables q{{q1_dev, q2_dev, q3_dev, q4_dev}};
    for (int n = 1; n <= 4; ++n)
        if (((order_mask >> (n - 1)) & 1) && !q.q[n - 1])
            return fail("esmk_op_ngram_energy: order " + std::to_string(n) + " is chosen but its table is null");
    ESMK_TRY(launch_ngram_energy(tokens_dev, code_dev, q, energy_out_dev, B, T, first, S, V, A, order_mask, (hipStream_t)stream));
    return 0;
}

int esmk_op_mh_accept_ex(int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* site_dev, const int32_t* tok_dev,
                         const int32_t* chain_id_dev, const double* e_contact_dev, const double* lp_sum_dev, const int32_t* n_res_dev,
                         const double* hastings_dev, const double* e_extra_dev, double w_contact, double w_lm, double w_extra,
                         const double* inv_t_dev, const int32_t* rung_dev, int n_rung, uint64_t seed, int step, double* e_cur_dev,
                         double* e_contact_cur_dev, double* e_lm_cur_dev, double* e_extra_cur_dev, uint8_t* accepted_out_dev,
                         double* u_out_dev, double* e_prop_out_dev, int n_chain, int B, int T, void* stream) {
    if (int rc = mh_accept_check("esmk_op_mh_accept_ex",
                                 !tokens_dev || !site_dev || !tok_dev || !chain_id_dev || !e_cur_dev || !accepted_out_dev || !inv_t_dev,
                                 lp_sum_dev, n_res_dev, n_chain, B, T))
        return rc;
    if (n_rung <= 0 || n_rung > ESMK_MAX_ROWS) return fail("esmk_op_mh_accept_ex: n_rung must be in 1 .. 2^24");
    if (!std::isfinite(w_contact) || !std::isfinite(w_lm) || !std::isfinite(w_extra))
        return fail("esmk_op_mh_accept_ex: the weights must be finite");
    if (step < 0) return fail("esmk_op_mh_accept_ex: step must not be negative");
    ESMK_TRY(launch_mh_accept(tokens_dev, slot_dev, site_dev, tok_dev, chain_id_dev, e_contact_dev, lp_sum_dev, n_res_dev, hastings_dev,
                              e_extra_dev, w_contact, w_lm, w_extra, inv_t_dev, /*inv_t0=*/0.0, rung_dev, n_rung,
                              (unsigned long long)seed, step, e_cur_dev, e_contact_cur_dev, e_lm_cur_dev, e_extra_cur_dev,
                              accepted_out_dev, u_out_dev, e_prop_out_dev, n_chain, B, T, (hipStream_t)stream));
    return 0;
}

int esmk_op_replica_swap(int32_t* rung_dev, const double* e_cur_dev, const double* inv_t_dev, const double* inv_t_host,
                         const int32_t* ladder_id_dev, uint64_t seed, int round, uint8_t* accepted_out_dev, double* u_out_dev,
                         int n_ladder, int K, void* stream) {
    if (!rung_dev || !e_cur_dev || !inv_t_dev || !inv_t_host || !ladder_id_dev || !accepted_out_dev || !u_out_dev)
        return fail("esmk_op_replica_swap: null argument");
    if (K < 1 || K > 64) return fail("esmk_op_replica_swap: K must be in 1 .. 64");
    if (n_ladder <= 0 || (long long)n_ladder * K > ESMK_MAX_ROWS) return fail("esmk_op_replica_swap: n_ladder * K must be in 1 .. 2^24");
    if (round < 0) return fail("esmk_op_replica_swap: round must not be negative");
    for (int k = 0; k < K; ++k)
        if (!(inv_t_host[k] >= 0.0) || std::isinf(inv_t_host[k]))
            return fail("esmk_op_replica_swap: every inv_t must be finite and not negative (a ladder has no greedy rung)");
    ESMK_TRY(launch_replica_swap(rung_dev, e_cur_dev, inv_t_dev, ladder_id_dev, (unsigned long long)seed, round, accepted_out_dev,
                                 u_out_dev, n_ladder, K, (hipStream_t)stream));
    return 0;
}

// ---- the token front end as single ops (tests/test_frontend_ops_gpu.py) -------------------------------------------
// Validation of what the engines guarantee their own calls, then the launchers of embed_stage (engine.hip), msa_embed_stage
// (engine_msa.hip), ensure_rope / ensure_sinus and the row gather of the scoring paths.  Segment tables arrive as host arrays
// and are checked with check_seg_table (lead_gap = false: the rules of esmk_forward_packed), uploaded, used and freed.
namespace {
constexpr long long kDynLdsDefault = 64 * 1024;  // dynamic LDS a kernel may ask for without hipFuncSetAttribute
constexpr long long kMaxIndex = 0x7fffffffLL - 256;  // int element indices of the kernels, rounded up to a workgroup

int bad_width(const std::string& w, const char* name, int E) {
    if (E <= 0 || E % 4 != 0) return fail(w + ": " + name + " must be a positive multiple of 4");
    return 0;
}
// (T + 4) ints of dynamic LDS: the position scan of add_positions_kernel / msa_embed_kernel
int bad_scan_row(const std::string& w, const char* name, int T, int D, int pad_idx, int npos) {
    if (npos <= 0 || pad_idx < 0) return fail(w + ": npos must be positive and pad_idx must not be negative");
    if (((long long)T + 4) * 4 > kDynLdsDefault)
        return fail(w + ": " + name + " needs (" + name + " + 4) * 4 bytes of dynamic LDS, above the default limit of 64 KiB");
    if (T > npos - pad_idx - 1) return fail(w + ": sequence length above the maximum of the positional embedding");
    if ((long long)T * (D / 4) > kMaxIndex) return fail(w + ": " + name + " * width / 4 exceeds 2^31");
    return 0;
}
int check_op_segments(const std::string& w, const int32_t* seg, int n_seg, int rows, SegTableInfo* info) {
    if (!seg) return fail(w + ": null segment table");
    return check_seg_table(w, seg, n_seg, rows, false, info);
}
int upload_segments(const int32_t* seg, int n_seg, DevBuf* d) {
    ESMK_TRY(hipMalloc(&d->p, (size_t)2 * n_seg * 4));
    ESMK_TRY(hipMemcpy(d->p, seg, (size_t)2 * n_seg * 4, hipMemcpyHostToDevice));
    return 0;
}
}  // namespace

int esmk_op_seq_stats(const int64_t* tokens_dev, int B, int T, int pad_idx, int mask_idx, int token_dropout, float* scale_dev,
                      float* key_bias_dev, int32_t* seq_info_dev, float* keep_dev, void* stream) {
    if (!tokens_dev || !scale_dev || !key_bias_dev || !seq_info_dev) return fail("esmk_op_seq_stats: null argument");
    if (B <= 0 || T <= 0) return fail("esmk_op_seq_stats: B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail("esmk_op_seq_stats: B*T exceeds 2^24 rows");
    ESMK_TRY(launch_seq_stats(tokens_dev, B, T, pad_idx, mask_idx, token_dropout, scale_dev, key_bias_dev, seq_info_dev,
                              (hipStream_t)stream, keep_dev));
    return 0;
}

int esmk_op_packed_stats(const int64_t* tokens_dev, const int32_t* segments_host, int n_seg, int rows, int pad_idx,
                         int mask_idx, float* scale_row_dev, float* key_bias_dev, int32_t* row_pos_dev, int32_t* seg_npad_dev,
                         float* keep_dev, void* stream) {
    const std::string w("esmk_op_packed_stats");
    if (!tokens_dev || !scale_row_dev || !key_bias_dev || !row_pos_dev || !seg_npad_dev) return fail(w + ": null argument");
    SegTableInfo info;
    if (check_op_segments(w, segments_host, n_seg, rows, &info)) return 1;
    DevBuf d;
    if (upload_segments(segments_host, n_seg, &d)) return 1;
    hipStream_t st = (hipStream_t)stream;
    ESMK_TRY(launch_packed_stats(tokens_dev, (const int*)d.p, n_seg, rows, pad_idx, mask_idx, scale_row_dev, key_bias_dev,
                                 row_pos_dev, seg_npad_dev, st, keep_dev));
    ESMK_TRY(hipStreamSynchronize(st));  // the table is freed on return
    return 0;
}

int esmk_op_zero_gap_rows(void* buf_dev, const int32_t* segments_host, int n_seg, int rows, size_t row_bytes, void* stream) {
    const std::string w("esmk_op_zero_gap_rows");
    if (!buf_dev) return fail(w + ": null argument");
    if (row_bytes == 0 || row_bytes % 16 != 0 || row_bytes > 0x7fffffff)
        return fail(w + ": row_bytes must be a positive multiple of 16 (below 2^31)");
    SegTableInfo info;
    if (check_op_segments(w, segments_host, n_seg, rows, &info)) return 1;
    DevBuf d;
    if (upload_segments(segments_host, n_seg, &d)) return 1;
    hipStream_t st = (hipStream_t)stream;
    ESMK_TRY(launch_zero_gap_rows(buf_dev, (const int*)d.p, n_seg, rows, row_bytes, st));
    ESMK_TRY(hipStreamSynchronize(st));  // the table is freed on return
    return 0;
}

int esmk_op_embed(const int64_t* tokens_dev, const float* table_dev, const float* scale_dev, float* x_dev, int B, int T, int E,
                  int vocab, int pad_idx, int mask_idx, int token_dropout, void* stream) {
    const std::string w("esmk_op_embed");
    if (!tokens_dev || !table_dev || !x_dev || (token_dropout && !scale_dev)) return fail(w + ": null argument");
    if (B <= 0 || T <= 0 || vocab <= 0) return fail(w + ": B, T and vocab must be positive");
    if (bad_width(w, "E", E)) return 1;
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    ESMK_TRY(launch_embed(tokens_dev, table_dev, scale_dev, x_dev, B, T, E, vocab, pad_idx, mask_idx, token_dropout,
                          (hipStream_t)stream));
    return 0;
}

int esmk_op_embed_esm1(const int64_t* tokens_dev, const float* table_dev, const float* scale_dev, const float* sinus_dev,
                       float* x_dev, int B, int T, int E, int vocab, int pad_idx, int mask_idx, int token_dropout,
                       float embed_scale, void* stream) {
    const std::string w("esmk_op_embed_esm1");
    if (!tokens_dev || !table_dev || !sinus_dev || !x_dev || (token_dropout && !scale_dev)) return fail(w + ": null argument");
    if (B <= 0 || T <= 0 || vocab <= 0) return fail(w + ": B, T and vocab must be positive");
    if (bad_width(w, "E", E)) return 1;
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    ESMK_TRY(launch_embed_esm1(tokens_dev, table_dev, scale_dev, sinus_dev, x_dev, B, T, E, vocab, pad_idx, mask_idx,
                               token_dropout, embed_scale, (hipStream_t)stream));
    return 0;
}

int esmk_op_add_positions(const int64_t* tokens_dev, const float* pos_emb_dev, float* x_dev, int B, int T, int E, int pad_idx,
                          int npos, const int32_t* segments_host, int n_seg, int rows, void* stream) {
    const std::string w("esmk_op_add_positions");
    if (!tokens_dev || !pos_emb_dev || !x_dev) return fail(w + ": null argument");
    if (B <= 0 || T <= 0) return fail(w + ": B and T must be positive");
    if (bad_width(w, "E", E)) return 1;
    if (bad_scan_row(w, "T", T, E, pad_idx, npos)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (segments_host == nullptr) {
        if (n_seg != 0 || rows != 0) return fail(w + ": n_seg and rows without a segment table");
        if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
        ESMK_TRY(launch_add_positions(tokens_dev, pos_emb_dev, x_dev, B, T, E, pad_idx, npos, st));
        return 0;
    }
    SegTableInfo info;
    if (check_op_segments(w, segments_host, n_seg, rows, &info)) return 1;
    if (B != n_seg || T < info.max_len)
        return fail(w + ": the packed form takes B = n_seg and T >= the longest segment (it sizes the LDS scan)");
    DevBuf d;
    if (upload_segments(segments_host, n_seg, &d)) return 1;
    ESMK_TRY(launch_add_positions(tokens_dev, pos_emb_dev, x_dev, n_seg, T, E, pad_idx, npos, st, (const int*)d.p));
    ESMK_TRY(hipStreamSynchronize(st));  // the table is freed on return
    return 0;
}

int esmk_op_scale_rows(float* x_dev, const float* keep_dev, int rows, int E, void* stream) {
    const std::string w("esmk_op_scale_rows");
    if (!x_dev || !keep_dev) return fail(w + ": null argument");
    if (rows <= 0 || rows > ESMK_MAX_ROWS) return fail(w + ": rows must be positive (at most 2^24)");
    if (bad_width(w, "E", E)) return 1;
    ESMK_TRY(launch_scale_rows(x_dev, keep_dev, rows, E, (hipStream_t)stream));
    return 0;
}

int esmk_op_msa_embed(const int64_t* tokens_dev, const float* tok_emb_dev, const float* pos_emb_dev, const float* msa_pos_dev,
                      float* x_dev, float* keep_dev, float* col_fill_dev, int32_t* any_pad_dev, int B, int R, int C, int D,
                      int vocab, int pad_idx, int npos, void* stream) {
    const std::string w("esmk_op_msa_embed");
    if (!tokens_dev || !tok_emb_dev || !pos_emb_dev || !x_dev || !keep_dev || !col_fill_dev || !any_pad_dev)
        return fail(w + ": null argument");
    if (B <= 0 || R <= 0 || C <= 0 || vocab <= 0) return fail(w + ": B, R, C and vocab must be positive");
    if (bad_width(w, "D", D)) return 1;
    if (bad_scan_row(w, "C", C, D, pad_idx, npos)) return 1;
    if ((long long)B * R * C > ESMK_MAX_ROWS) return fail(w + ": B*R*C exceeds 2^24 rows");
    ESMK_TRY(launch_msa_embed(tokens_dev, tok_emb_dev, pos_emb_dev, msa_pos_dev, x_dev, keep_dev, col_fill_dev, any_pad_dev, B, R,
                              C, D, vocab, pad_idx, npos, (hipStream_t)stream));
    return 0;
}

int esmk_op_sinus_table(const float* freq_dev, float* table_dev, int T, int half, int pos0, void* stream) {
    if (!freq_dev || !table_dev) return fail("esmk_op_sinus_table: null argument");
    if (T <= 0 || half <= 0) return fail("esmk_op_sinus_table: T and half must be positive");
    if ((long long)T * half > kMaxIndex) return fail("esmk_op_sinus_table: T * half exceeds 2^31");
    ESMK_TRY(launch_sinus_table(freq_dev, table_dev, T, half, pos0, (hipStream_t)stream));
    return 0;
}

int esmk_op_rope_table(const float* inv_freq_dev, float* cos_dev, float* sin_dev, int T, int half, void* stream) {
    if (!inv_freq_dev || !cos_dev || !sin_dev) return fail("esmk_op_rope_table: null argument");
    if (T <= 0 || half <= 0) return fail("esmk_op_rope_table: T and half must be positive");
    if ((long long)T * half > kMaxIndex) return fail("esmk_op_rope_table: T * half exceeds 2^31");
    ESMK_TRY(launch_rope_table(inv_freq_dev, cos_dev, sin_dev, T, half, (hipStream_t)stream));
    return 0;
}

int esmk_op_gather_rows(const float* x_dev, const int32_t* sel_dev, float* out_dev, int N, int E, int n, void* stream) {
    const std::string w("esmk_op_gather_rows");
    if (!x_dev || !sel_dev || !out_dev) return fail(w + ": null argument");
    if (N <= 0 || n <= 0 || N > ESMK_MAX_ROWS || n > ESMK_MAX_ROWS) return fail(w + ": N and n must be positive (at most 2^24)");
    if (bad_width(w, "E", E)) return 1;
    ESMK_TRY(launch_gather_rows(x_dev, sel_dev, out_dev, N, E, n, (hipStream_t)stream));
    return 0;
}

int esmk_op_contacts(const float* attn_dev, const int64_t* tokens_dev, const float* w_dev,
                     const float* b_dev, float* scratch_dev, float* out_dev, int B, int C, int T,
                     int eos_idx, int prepend_bos, int append_eos, void* stream) {
    ESMK_TRY(launch_contacts(attn_dev, tokens_dev, w_dev, b_dev, scratch_dev, out_dev, B, C, T,
                             eos_idx, prepend_bos, append_eos, (hipStream_t)stream));
    return 0;
}

}  // extern "C"

