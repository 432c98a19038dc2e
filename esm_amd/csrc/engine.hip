// engine.hip — the C ABI of libesmk.so (declared in include/esmk.h): parameter packing,
// workspace planning and the launch sequence that replaces ESM2.forward
// (reference esm/model/esm2.py:77-144).  Host code only; every kernel lives in gemm.hip,
// attention.hip and elementwise.hip.
#include "engine_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

using namespace esmk;
using namespace esmk_host;

// LayerNorm fold for handles created with esmk_config::ln_fold == 0 and no ESMK_LN_FOLD in the environment:
// ON since round 5 wherever the configuration supports it (plain fp16 / bf16 operands, head_dim <= 64) — faster at every
// batch size (B = 64 + 1.1 %, B = 4 + 6.5 %) and on the fp16-operand floor numerically, like the plain mode
static constexpr bool kLnFoldDefault = true;

namespace {
thread_local std::string g_err;
}

namespace esmk_host {
int fail(const char* what, hipError_t e) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return 1;
}
int fail(const std::string& msg) {
    g_err = msg;
    return 1;
}
}  // namespace esmk_host

namespace {

void plan_packed(esmk_model* m) {
    const size_t os = op_size(m->cfg.operand_dtype);
    const size_t E = m->E, F = m->F, V = m->V, EA = m->EA, Kp = m->Kp;
    // f16x2: every layer matrix as [rows, 2 cols] (hi | lo K tiles); f16x2a (weight_split 2): the attention projections only
    const size_t ws = m->cfg.weight_split ? 2 : 1;
    const SplitPlan sp = split_plan(m);
    Carve c;
    m->embed_f32 = c.take(V * E * 4);
    m->embed_op = c.take(V * Kp * os);
    m->fin_g = c.take(E * 4);
    m->fin_b = c.take(E * 4);
    m->lm_w = c.take(E * Kp * os);
    m->lm_w32 = c.take(ws == 2 ? E * E * 4 : 0);
    m->lm_b = c.take(E * 4);
    m->lm_lng = c.take(E * 4);
    m->lm_lnb = c.take(E * 4);
    m->lm_bias = c.take(V * 4);
    m->ct_w = c.take((size_t)m->L * m->H * 4);
    m->ct_b = c.take(4);
    if (m->cfg.num_positions > 0) m->pos_emb = c.take((size_t)m->cfg.num_positions * E * 4);
    if (m->cfg.ln_before) {
        m->lnb_g = c.take(E * 4);
        m->lnb_b = c.take(E * 4);
    }
    m->layer.resize(m->L);
    for (int l = 0; l < m->L; ++l) {
        LayerOff& o = m->layer[l];
        o.wqkv = c.take(EA * Kp * os * (2 * sp.qk + sp.v));   // q, k rows | v rows (each block with its own row length)
        o.bqkv = c.take(3 * EA * 4);
        o.wo = c.take(E * EA * os * sp.o);
        o.bo = c.take(E * 4);
        o.w1 = c.take(F * Kp * os * sp.ffn);
        o.b1 = c.take(F * 4);
        o.w2 = c.take(E * F * os * sp.ffn);
        o.b2 = c.take(E * 4);
        o.ln1g = c.take(E * 4);
        o.ln1b = c.take(E * 4);
        o.ln2g = c.take(E * 4);
        o.ln2b = c.take(E * 4);
        if (m->fold) {
            o.bqkv2 = c.take(3 * EA * 4);
            o.b12 = c.take(F * 4);
        }
        if (m->esm1) o.bkv = c.take(2 * EA * os);
    }
    if (m->esm1) {
        m->out_w = c.take(V * Kp * os);
        m->out_b = c.take(V * 4);
    }
    m->packed_bytes = c.off;
}

struct Workspace {
    size_t scale, key_bias, seq_info, keep, x, h, big, lse, ct_scratch, total;
    size_t h2 = 0, ln_part = 0, ln_mean = 0, ln_rstd = 0;  // LayerNorm fold
    int ln_parts = 0;
    size_t a3 = 0, ffn3 = 0;  // precision mode f16x3: hi | hi | lo operand rows (LayerNorm output / attention context; fc1 + GELU output)
    size_t ct_acc, ct_row, ct_col, ct_rowp, ct_colp, ct_wt;  // contacts without attention maps (contacts.hip)
    size_t q, k, vt;  // inside big
    int Tp;
    size_t row_pos, tables;  // token-packed batches only
};

// Token-packed batch (esmk_forward_packed): ONE row space of `rows` rows holding n_seg segments.  The layer
// stack sees it as B = 1, T = rows; only three kernels know about segments (token statistics, the rotary
// position in the q/k epilogue, the attention kernel's key range).
struct PackedCtx {
    int n_seg = 0, max_len = 0, n_items = 0;
    unsigned long long sum_len2 = 0;    // sum of len^2: the attention work
    const int32_t* seg_host = nullptr;  // [n_seg][2] = (first row, length)
    const CtPackedPlan* ct = nullptr;   // contacts (esmk_forward_packed_ex): scratch sizes and work lists
    // attention maps (esmk_forward_packed_maps): ragged [L, H, len, len] blocks in maps_out, fp32 or the operand dtype
    bool maps = false, maps_lowp = false;
    void* maps_out = nullptr;
};
// Row selection (esmk_forward_rows): the layer stack runs on all B*T rows, the head of the model — final LayerNorm, LM head,
// vocabulary GEMM — on the n_sel gathered rows only, and a log-softmax turns their logits into logprobs_out.  The gathered
// rows and the head's intermediates live behind the forward's own workspace (plan_rows).
struct RowSel {
    const int32_t* sel_dev = nullptr;  // int32 [n_sel] flat row indices b*T + t, device data: clamped by the gather kernel
    int n_sel = 0;
    float* logprobs_out = nullptr;     // fp32 [n_sel, V]
    size_t x = 0, h = 0, g32 = 0, logits = 0;  // byte offsets into the workspace
};
// query blocks of 128 rows: sum over segments of ceil(len / 128) <= rows / 128 + n_seg
inline size_t packed_items_bound(int n_seg, int rows) { return (size_t)rows / 128 + (size_t)n_seg; }

// ct: token-packed batch with ESMK_OUT_CONTACTS (flags must then hold it): per-segment contact scratch
// packed_maps: token-packed batch with attention maps: lse and the 64-bit map offsets; nothing that grows with Tmax^2
// ct_G > 0: the head-group count of the fused contact accumulators is given (esmk_forward_rows_contacts pins it to B = 1's)
Workspace plan_workspace(const esmk_model* m, int B, int T, uint32_t flags, int packed_segs = 0,
                         const CtPackedPlan* ct = nullptr, bool packed_maps = false, int ct_G = 0) {
    Workspace w{};
    const size_t os = op_size(m->cfg.operand_dtype);
    const size_t N = (size_t)B * T, E = m->E, F = m->F, EA = m->EA, Kp = m->Kp;
    // packed: one spare (zeroed) key tile behind the rows, because a segment's last 64-key tile may start
    // anywhere and reach past the last row
    w.Tp = (T + 63) / 64 * 64 + (packed_segs > 0 ? 64 : 0);
    Carve c;
    w.scale = c.take((packed_segs > 0 ? N : (size_t)B) * 4);
    w.key_bias = c.take(N * 4);
    w.seq_info = c.take((size_t)B * 2 * 4);
    w.keep = c.take(m->cfg.num_positions > 0 ? N * 4 : 0);
    w.x = c.take(N * E * 4);
    w.h = c.take(N * std::max(Kp, EA) * os);
    if (m->fold) {
        // h: the raw rows of the residual stream in the operand dtype (A operand of q/k/v and fc1), h2: the attention
        // context; statistics per row, padded to whole 256-row tiles (the V^T epilogue loads four rows at a time)
        const size_t Np = (N + 255) / 256 * 256;
        w.ln_parts = (int)((E + 127) / 128);
        w.h2 = c.take(N * std::max(Kp, EA) * os);
        w.ln_part = c.take(Np * w.ln_parts * 2 * 4);
        w.ln_mean = c.take(Np * 4);
        w.ln_rstd = c.take(Np * 4);
    }
    if (split_x3(m)) {
        w.a3 = c.take(N * 3 * std::max(Kp, EA) * os);
        w.ffn3 = c.take(N * 3 * F * os);
    }
    const size_t qb = align_up(N * EA * os);
    const size_t vtb = align_up((size_t)B * EA * w.Tp * os);
    size_t big = 2 * qb + vtb;
    if (N * F * os > big) big = N * F * os;
    if (N * E * 4 > big) big = N * E * 4;
    w.big = c.take(big);
    w.q = w.big;
    w.k = w.big + qb;
    w.vt = w.big + 2 * qb;
    const bool attn = (flags & (ESMK_OUT_ATTN | ESMK_OUT_CONTACTS)) || packed_maps;
    w.lse = c.take(attn ? (size_t)B * m->H * T * 4 : 0);
    const int S = T - (m->cfg.prepend_bos ? 1 : 0) - (m->cfg.append_eos ? 1 : 0);
    // ESMK_OUT_CONTACTS without ESMK_OUT_ATTN: no [B,L,H,T,T] tensor anywhere (contacts.hip)
    const bool fused_ct = (flags & ESMK_OUT_CONTACTS) && !(flags & ESMK_OUT_ATTN);
    w.ct_scratch = c.take(((flags & ESMK_OUT_CONTACTS) && !fused_ct)
                              ? (size_t)B * m->L * m->H * (size_t)(S > 0 ? S + 1 : 1) * 4 : 0);
    const size_t C = (size_t)m->L * m->H;
    const long long nQ = (T + 127) / 128;
    if (ct != nullptr) {  // per segment: G x len^2 accumulators, [C, len] sums, row / column partials (contacts.hip)
        w.ct_acc = c.take((size_t)ct->G * ct->sum_len2 * 4);
        w.ct_row = c.take((size_t)C * T * 4);
        w.ct_col = c.take((size_t)C * T * 4);
        w.ct_rowp = c.take((size_t)ct->rowp * 4);
        w.ct_colp = c.take((size_t)ct->colp * 4);
        w.ct_wt = c.take((size_t)packed_segs * C * 4);
    } else {
        const int G = ct_G > 0 ? ct_G : contacts_head_groups((long long)B * nQ * nQ, m->H, head_slots(m));
        w.ct_acc = c.take(fused_ct ? (size_t)G * B * T * T * 4 : 0);
        w.ct_row = c.take(fused_ct ? (size_t)B * C * T * 4 : 0);
        w.ct_col = c.take(fused_ct ? (size_t)B * C * T * 4 : 0);
        w.ct_rowp = c.take(fused_ct ? (size_t)B * ((T + 127) / 128) * m->H * T * 4 : 0);
        w.ct_colp = c.take(fused_ct ? (size_t)B * ((T + 31) / 32) * m->H * T * 4 : 0);
        w.ct_wt = c.take(fused_ct ? (size_t)B * C * 4 : 0);
    }
    if (packed_segs > 0) {
        w.row_pos = c.take(N * 4);
        // the tables are planned for the upper bound of the work list (packed_tables: the layout)
        w.tables = c.take(packed_tables(packed_segs, packed_items_bound(packed_segs, T), ct ? ct->table_ints() : 0, packed_maps).ints * 4);
    }
    w.total = c.off;
    return w;
}

// esmk_forward_rows: the forward's workspace, then the selected rows of the stream (fp32), their operand-dtype rows, the fp32
// scratch of the head and the selected logits.  No pad rows: every GEMM kernel clamps its A-row reads to row M - 1 and stores
// rows below M only, so M = n_sel is launched as it is.
// packed_segs > 0 (esmk_forward_packed_rows): the token-packed forward's workspace (B = 1, T = rows) in front.
// flags, ct_G (esmk_forward_rows_contacts): the forward in front also accumulates contact maps, with ct_G head groups.
size_t plan_rows(const esmk_model* m, int B, int T, int n_sel, RowSel* rs, int packed_segs = 0,
                 uint32_t flags = ESMK_OUT_LOGITS, int ct_G = 0) {
    Carve c;
    c.take(plan_workspace(m, B, T, flags, packed_segs, nullptr, false, ct_G).total);
    const size_t n = (size_t)n_sel;
    rs->x = c.take(n * m->E * 4);
    rs->h = c.take(n * std::max(m->Kp, m->EA) * op_size(m->cfg.operand_dtype));
    rs->g32 = c.take(n * m->E * 4);
    rs->logits = c.take(n * m->V * 4);
    return c.off;
}

// esmk_forward_rows_pair: behind plan_rows' layout, every layer's q, k [L][B,H,T,slots] (operand dtype) and row log-sum-exp
// [L][B,H,T]: the stacked operands of launch_pair_head.  A layer's q / k / lse outputs point at its slot.
struct PairStash {
    size_t q = 0, k = 0, lse = 0;      // byte offsets into the workspace
    size_t qk_layer = 0, lse_layer = 0;  // bytes per layer
    float* out = nullptr;              // fp32 [B,S,S,n_sym + n_asym]
};
size_t plan_rows_pair(const esmk_model* m, int B, int T, int n_sel, RowSel* rs, PairStash* ps) {
    Carve c;
    c.take(plan_rows(m, B, T, n_sel, rs));
    const size_t N = (size_t)B * T;
    ps->qk_layer = N * m->EA * op_size(m->cfg.operand_dtype);
    ps->lse_layer = (size_t)B * m->H * T * 4;
    ps->q = c.take(ps->qk_layer * m->L);
    ps->k = c.take(ps->qk_layer * m->L);
    ps->lse = c.take(ps->lse_layer * m->L);
    return c.off;
}

// ESM-1: the sinusoidal position table for rows 0 .. T-1 (SinusoidalPositionalEmbedding.get_embedding, modules.py:283-295).
// The half frequencies exp(j * -(ln 10000 / (half - 1))) are fp32 values of an fp32 argument, as the reference computes them
// (correctly rounded here); angles, sin and cos on the device (sinus_table_kernel).
int ensure_sinus(esmk_model* m, int T, hipStream_t st) {
    if (T <= m->sinus_cap) return 0;
    int cap = 1024;
    while (cap < T) cap *= 2;
    if (m->d_sinus) {
        ESMK_TRY(hipStreamSynchronize(st));
        ESMK_TRY(hipFree(m->d_sinus));
        m->d_sinus = nullptr;
        m->sinus_cap = 0;
    }
    const int half = m->E / 2;
    std::vector<float> freq(half);
    const float step = (float)(-(log(10000.0) / (double)(half - 1)));
    for (int j = 0; j < half; ++j) freq[j] = (float)exp((double)((float)j * step));
    float* d_freq = nullptr;
    ESMK_TRY(hipMalloc(&m->d_sinus, (size_t)cap * m->E * 4));
    ESMK_TRY(hipMalloc(&d_freq, (size_t)half * 4));
    ESMK_TRY(hipMemcpy(d_freq, freq.data(), (size_t)half * 4, hipMemcpyHostToDevice));
    ESMK_TRY(launch_sinus_table(d_freq, m->d_sinus, cap, half, m->cfg.pad_idx + 1, st));
    ESMK_TRY(hipStreamSynchronize(st));
    ESMK_TRY(hipFree(d_freq));
    m->sinus_cap = cap;
    return 0;
}

}  // namespace

__global__ void fill_f32_kernel(float* p, float v, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

namespace esmk_host {
int g_rows_contacts_own_groups = 0;

int ensure_rope(esmk_model* m, int T, hipStream_t st) {
    if (m->inv_freq.empty()) return fail("esmk_set_rope_inv_freq was not called");
    if (T <= m->rope_cap) return 0;
    int cap = 1024;
    while (cap < T) cap *= 2;
    const int half = m->D == 128 ? 64 : 32;
    if (m->d_cos) {
        ESMK_TRY(hipStreamSynchronize(st));
        ESMK_TRY(hipFree(m->d_cos));
        ESMK_TRY(hipFree(m->d_sin));
        m->d_cos = m->d_sin = nullptr;
        m->rope_cap = 0;
    }
    ESMK_TRY(hipMalloc(&m->d_cos, (size_t)cap * half * 4));
    ESMK_TRY(hipMalloc(&m->d_sin, (size_t)cap * half * 4));
    ESMK_TRY(launch_rope_table(m->d_inv_freq, m->d_cos, m->d_sin, cap, half, st));
    m->rope_cap = cap;
    return 0;
}

int ensure_unit_rope(esmk_model* m, int T, hipStream_t st) {
    if (T <= m->unit_cap) return 0;
    int cap = 1024;
    while (cap < T) cap *= 2;
    if (m->d_ucos) {
        ESMK_TRY(hipStreamSynchronize(st));
        ESMK_TRY(hipFree(m->d_ucos));
        ESMK_TRY(hipFree(m->d_usin));
        m->d_ucos = m->d_usin = nullptr;
        m->unit_cap = 0;
    }
    const size_t n = (size_t)cap * 64;  // row stride 32 (head_dim <= 64) or 64 (head_dim 128)
    ESMK_TRY(hipMalloc(&m->d_ucos, n * 4));
    ESMK_TRY(hipMalloc(&m->d_usin, n * 4));
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->d_ucos, 1.0f, n);
    ESMK_TRY(hipGetLastError());
    ESMK_TRY(hipMemsetAsync(m->d_usin, 0, n * 4, st));
    m->unit_cap = cap;
    return 0;
}

int Stack::gemm(int cls, const GemmArgs& a, int epi, double out_bytes_per_elem) const {
    const double z = a.batch > 0 ? a.batch : 1;
    const double fl = 2.0 * z * a.M * (double)(a.n_valid ? a.n_valid : a.N) * a.K;
    const double by = z * (((double)a.M * a.K + (double)a.N * a.K) * os + (double)a.M * a.N * out_bytes_per_elem);
    ProfScope ps(m, st, cls, fl, by);
    ESMK_TRY(launch_gemm(a, epi, op, st));
    return 0;
}

int Stack::weight_gemm(int cls, GemmArgs a, int epi, double out_bytes_per_elem) const {
    if (split_factor(m, cls, epi) == 1) return gemm(cls, a, epi, out_bytes_per_elem);
    const double fl = 2.0 * a.M * (double)a.N * a.K;
    const double by = ((double)a.M * a.K + 2.0 * a.N * a.K) * os + (double)a.M * a.N * out_bytes_per_elem;
    a.a_row_bytes = (long long)a.K * (long long)os;
    a.a_kt_repeat = 1;
    a.K *= 2;
    ProfScope ps(m, st, cls, fl, by);
    ESMK_TRY(launch_gemm(a, epi, op, st));
    return 0;
}

int Stack::lnorm(const float* in, size_t gamma_off, size_t beta_off, void* y, float* y32, int rows, const LnExtra& ex) const {
    const double RE = (double)rows * m->E;
    ProfScope ps(m, st, PC_LAYERNORM, 8 * RE, RE * (4 + (y ? os * (ex.x3 ? 3 : 1) : 0) + (y32 ? 4 : 0)));
    ESMK_TRY(launch_layernorm_ex(in, (const float*)(pk + gamma_off), (const float*)(pk + beta_off), y, y32, rows, m->E, op, ex, st));
    return 0;
}

int Stack::repr_copy(int layer, const float* src, bool lowp) const {
    const size_t n = (size_t)N * m->E;
    for (int i = 0; i < n_repr; ++i)
        if (repr_layers[i] == layer) {
            ProfScope ps(m, st, PC_COPY, 0, (lowp ? 4 + os : 8) * (double)n);
            if (lowp) ESMK_TRY(launch_convert(src, ESMK_DT_F32, repr_out[i], op, n, st));
            else ESMK_TRY(launch_copy_f32(src, (float*)repr_out[i], n, st));
        }
    return 0;
}

int lm_head(const Stack& s, int rows, float* x, void* h, float* g32, int Kp, const LnExtra& ex, bool repr_lowp,
            bool want_logits, void* logits_out) {
    const esmk_model* m = s.m;
    const int E = m->E, V = m->V;
    float* rep_last = (float*)s.repr_of(m->L);
    const bool normed = repr_lowp && rep_last != nullptr;  // by the caller, into h and the operand-dtype representation
    if (repr_lowp) rep_last = nullptr;
    if (!normed && (want_logits || rep_last != nullptr)) {
        if (s.lnorm(x, m->fin_g, m->fin_b, want_logits ? h : nullptr, rep_last, rows, ex)) return 1;
        for (int i = 0; i < s.n_repr; ++i)  // duplicates of layer L, if any
            if (s.repr_layers[i] == m->L && s.repr_out[i] != rep_last)
                ESMK_TRY(launch_copy_f32(rep_last, (float*)s.repr_out[i], (size_t)s.N * E, s.st));
    }
    if (!want_logits) return 0;
    if (m->cfg.weight_split && E % 32 == 0) {
        // f16x2 precision mode: two small fp32 GEMMs per forward; neither the head's weights nor its activations are
        // rounded to fp16, so the logits carry only the error of the representation itself
        const double RE = (double)rows * E;
        float* a32 = rep_last != nullptr ? rep_last : g32;
        if (a32 == g32 && s.lnorm(x, m->fin_g, m->fin_b, nullptr, g32, rows, ex)) return 1;  // the normalised stream in fp32
        {
            ProfScope ps(s.m, s.st, PC_LM_DENSE, 2.0 * rows * (double)E * E, (2.0 * RE + (double)E * E) * 4);
            ESMK_TRY(launch_gemm32(a32, E, (const float*)(s.pk + m->lm_w32), (const float*)(s.pk + m->lm_b), x, E, rows, E, E, true, s.st));
        }
        if (s.lnorm(x, m->lm_lng, m->lm_lnb, nullptr, g32, rows, ex)) return 1;  // x (the residual stream) is dead: dense output
        ProfScope ps(s.m, s.st, PC_LM_LOGITS, 2.0 * rows * (double)E * V, (RE + (double)V * E + (double)rows * V) * 4);
        ESMK_TRY(launch_gemm32(g32, E, (const float*)(s.pk + m->embed_f32), (const float*)(s.pk + m->lm_bias), (float*)logits_out, V,
                               rows, V, E, false, s.st));
        return 0;
    }
    GemmArgs g;
    g.A = h;
    g.W = s.pk + m->lm_w;
    g.bias = (const float*)(s.pk + m->lm_b);
    g.out = g32;
    g.M = rows;
    g.N = E;
    g.K = Kp;
    if (s.gemm(PC_LM_DENSE, g, EPI_GELU_F32, 4)) return 1;
    if (s.lnorm(g32, m->lm_lng, m->lm_lnb, h, nullptr, rows, ex)) return 1;
    g = GemmArgs();
    g.A = h;
    g.W = s.pk + m->embed_op;
    g.bias = (const float*)(s.pk + m->lm_bias);
    g.out = logits_out;
    g.M = rows;
    g.N = V;
    g.K = Kp;
    return s.gemm(PC_LM_LOGITS, g, EPI_STORE_F32, 4);
}

void qkv_gemm_args(const esmk_model* m, const QkvProj& p, GemmArgs* qk, GemmArgs* v) {
    const int EA = m->EA;
    GemmArgs g;
    g.A = p.A;
    g.W = p.W;
    g.bias = p.bias;
    g.bias2 = p.bias2;
    g.ln_rstd = p.ln_rstd;
    g.M = p.rows;
    g.N = 2 * EA;  // q, k: weight rows [0, 2 EA)
    g.K = p.K;
    g.q = p.q;
    g.k = p.k;
    g.vt = p.vt;
    g.cos = p.cos;
    g.sin = p.sin;
    g.T = p.T;
    g.H = m->H;
    g.E = EA;
    g.Tp = p.Tp;
    g.scaling = p.scaling;
    g.head_dim = head_slots(m);
    *v = g;
    g.row_pos = p.row_pos;
    g.row_keep = p.row_keep;
    *qk = g;
    v->W = (const char*)p.W + (size_t)2 * EA * m->Kp * op_size(m->cfg.operand_dtype) * p.split;  // v: weight rows [2 EA, 3 EA)
    v->bias = p.bias + 2 * EA;
    if (p.bias2) v->bias2 = p.bias2 + 2 * EA;
    v->N = EA;
    v->vt_rows = p.vt_rows;
}

int check_seg_table(const std::string& w, const int32_t* seg, int n_seg, int rows, bool lead_gap, SegTableInfo* info) {
    if (n_seg <= 0 || rows <= 0) return fail(w + ": n_seg and rows must be positive");
    if (rows % 64 != 0) return fail(w + ": rows must be a multiple of 64");
    if (rows > ESMK_MAX_ROWS) return fail(w + ": rows exceed 2^24");
    long long end = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int start = seg[2 * s], len = seg[2 * s + 1];
        if (len <= 0) return fail(w + ": empty segment");
        if (start % 16 != 0) return fail(w + ": segment starts must be multiples of 16");
        if ((s == 0 && start != 0 && !lead_gap) || start < end)
            return fail(w + (lead_gap ? ": segments must be ascending and disjoint" : ": segments must start at row 0, ascending, disjoint"));
        end = (long long)start + len;
        if (end > rows) return fail(w + ": segment past the last row");
        info->max_len = std::max(info->max_len, len);
        info->items += (size_t)(len + 127) / 128;
        info->sum_len2 += (unsigned long long)len * (unsigned long long)len;
    }
    return 0;
}
// dst: [seg 2 n][npad n (zero: filled on the device)][work 4 items] — query blocks of 128 rows, longest segments first: the
// tail of the grid is made of short work items
void fill_attn_tables(const int32_t* seg, int n_seg, int32_t* dst) {
    memcpy(dst, seg, (size_t)2 * n_seg * 4);
    memset(dst + (size_t)2 * n_seg, 0, (size_t)n_seg * 4);
    std::vector<int> order(n_seg);
    for (int s = 0; s < n_seg; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return seg[2 * a + 1] > seg[2 * b + 1]; });
    int32_t* wk = dst + (size_t)3 * n_seg;
    for (int s : order) {
        const int start = seg[2 * s], len = seg[2 * s + 1];
        for (int q0 = 0; q0 < len; q0 += 128) {
            wk[0] = start;
            wk[1] = len;
            wk[2] = q0;
            wk[3] = s;
            wk += 4;
        }
    }
}
// dst: uint64 [n_seg] (as int32 pairs, 8-byte aligned): map offset of segment s = sum of len^2 of the segments in front
void fill_map_offsets(const int32_t* seg, int n_seg, int32_t* dst) {
    unsigned long long acc = 0;
    for (int s = 0; s < n_seg; ++s) {
        memcpy(dst + 2 * (size_t)s, &acc, 8);
        acc += (unsigned long long)seg[2 * s + 1] * (unsigned long long)seg[2 * s + 1];
    }
}


int check_stream_edit(const std::string& w, const esmk_stream_edit& e, int E, int L) {
    if (L >= 0 && (e.layer < 0 || e.layer > L))
        return fail(w + ": layer " + std::to_string(e.layer) + " is outside 0 .. " + std::to_string(L) + " (the stream after that many layers)");
    if (e.op != ESMK_EDIT_AXPBY && e.op != ESMK_EDIT_PROJECT) return fail(w + ": op must be ESMK_EDIT_AXPBY or ESMK_EDIT_PROJECT");
    if (e.op == ESMK_EDIT_PROJECT && !e.src_dev) return fail(w + ": ESMK_EDIT_PROJECT needs src_dev (the direction)");
    if (e.rows_dev && e.n_rows < 0) return fail(w + ": n_rows must not be negative");
    if (e.rows_dev && e.n_rows > ESMK_MAX_ROWS) return fail(w + ": n_rows exceeds 2^24 rows");
    if (e.src_dev && e.src_ld != 0 && (e.src_ld < E || e.src_ld % 4 != 0))
        return fail(w + ": src_ld must be 0 (one vector for every row) or a multiple of 4 that is >= embed_dim");
    if (e.src_dev && e.src_ld != 0 && e.n_src <= 0) return fail(w + ": n_src must be positive when src_ld is a row stride");
    if (E % 4 != 0 || E > 5120) return fail(w + ": the edit kernel takes embed_dim % 4 == 0, embed_dim <= 5120");
    return 0;
}

}  // namespace esmk_host

namespace {

bool starts_with(const char* s, const char* p) { return strncmp(s, p, strlen(p)) == 0; }

size_t numel(const int64_t* shape, int ndim) {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    return n;
}

}  // namespace

// =============================================================================================
// The forward of ESM-2 / ESM-1b / ESM-1 (esmk_forward and its row-selected and token-packed forms), in stages
// =============================================================================================
namespace {

// One call, as the entries fill it in
struct ForwardCall {
    const char* who = "esmk_forward";  // every message names this entry
    esmk_model* m = nullptr;
    const void* packed = nullptr;
    const int64_t* tokens = nullptr;
    int B = 0, T = 0;
    const int32_t* repr_layers = nullptr;
    int n_repr = 0;
    void* const* repr_out = nullptr;
    uint32_t flags = 0;
    void *logits = nullptr, *attn = nullptr, *contacts = nullptr, *workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
    const PackedCtx* pc = nullptr;  // token-packed batch: B = 1, T = rows
    const RowSel* rs = nullptr;     // esmk_forward_rows, esmk_forward_packed_rows, esmk_forward_rows_contacts
    int ct_G = 0;                   // esmk_forward_rows_contacts: the pinned head-group count of the fused contact head (0: from B)
    const PairStash* ps = nullptr;  // esmk_forward_rows_pair: the q / k / lse stash behind the workspace and the head's output
};

// What the stages share: the call, the launch helpers, the workspace and the form the model runs in
struct Fwd {
    const ForwardCall& c;
    esmk_model* const m;
    const PackedCtx* const pc;
    const Workspace w;
    const int B, T, N, E, F, H, L, EA, Kp;
    const Stack s;
    const bool want_logits, want_contacts, want_attn, fused_ct, repr_lowp, attn_lowp, packed_maps;
    const int S_ct;
    // LayerNorm fold; precision mode f16x3 (weight_split 4): every layer GEMM is a PLAIN launch over
    // K' = 3 K — weight images hi | lo | hi per K tile against operand rows hi | hi | lo; ESM-1
    const bool fold, x3, esm1;
    const int kx;  // operand columns per K column: 3 in the f16x3 mode
    char* const ws;
    float *scale, *key_bias, *x, *g32, *lse;
    int* seq_info;
    void *h, *q, *k, *vt;
    // Operand rows of the layer GEMMs.  act: the normalised stream (q / k / v, fc1) — with the fold the raw rows of the
    // stream in the operand dtype (written by rowstats for layer 0, then by the residual epilogues); ctx: the attention
    // context (out_proj); ffn: fc1's output (fc2).  f16x3: the hi | hi | lo rows a3 (LnExtra::x3 and the attention kernel's
    // X3 output) and ffn3 (GemmArgs::x3_out)
    void *act, *ctx, *ffn;
    float *ln_part = nullptr, *ln_mean = nullptr, *ln_rstd = nullptr;  // fold
    // token-packed batch: the tables behind the workspace (upload_packed_tables)
    int* row_pos = nullptr;
    AttnSegs segs;
    CtPackedDev ctd;
    const unsigned long long* map_off = nullptr;  // packed attention maps: sum of len^2 of the segments in front

    Fwd(const ForwardCall& c_, const Workspace& w_)
        : c(c_), m(c_.m), pc(c_.pc), w(w_), B(c_.B), T(c_.T), N(c_.B * c_.T), E(m->E), F(m->F), H(m->H), L(m->L), EA(m->EA),
          Kp(m->Kp),
          s{m, (hipStream_t)c_.stream, m->cfg.operand_dtype, op_size(m->cfg.operand_dtype), (const char*)c_.packed, N,
            c_.repr_layers, c_.n_repr, c_.repr_out},
          want_logits(c_.flags & ESMK_OUT_LOGITS), want_contacts(c_.flags & ESMK_OUT_CONTACTS),
          want_attn(c_.flags & ESMK_OUT_ATTN),
          // contacts alone (predict_contacts, esm2.py:146-147): accumulated layer by layer, no attention tensor
          fused_ct(want_contacts && !want_attn), repr_lowp(c_.flags & ESMK_OUT_REPR_LOWP),
          attn_lowp(c_.flags & ESMK_OUT_ATTN_LOWP), packed_maps(pc != nullptr && pc->maps),
          S_ct(T - (m->cfg.prepend_bos ? 1 : 0) - (m->cfg.append_eos ? 1 : 0)), fold(m->fold), x3(split_x3(m)),
          esm1(m->esm1 != 0), kx(x3 ? 3 : 1), ws((char*)c_.workspace) {
        scale = (float*)(ws + w.scale);
        key_bias = (float*)(ws + w.key_bias);
        seq_info = (int*)(ws + w.seq_info);
        x = (float*)(ws + w.x);
        h = ws + w.h;
        q = ws + w.q;
        k = ws + w.k;
        vt = ws + w.vt;
        g32 = (float*)(ws + w.big);
        lse = (want_attn || fused_ct || packed_maps) ? (float*)(ws + w.lse) : nullptr;
        act = x3 ? ws + w.a3 : h;
        ctx = x3 ? ws + w.a3 : fold ? ws + w.h2 : h;
        ffn = x3 ? ws + w.ffn3 : ws + w.big;
        if (fold) {
            ln_part = (float*)(ws + w.ln_part);
            ln_mean = (float*)(ws + w.ln_mean);
            ln_rstd = (float*)(ws + w.ln_rstd);
        }
    }
    std::string who() const { return c.who; }
    template <typename T_>
    T_* at(size_t off) const { return (T_*)(ws + off); }
    const float* param(size_t off) const { return (const float*)(s.pk + off); }

    // a GEMM of the layer stack: f16x3 launches it as it is, the f16x2 modes over the split image
    int layer_gemm(int cls, const GemmArgs& g, int epi, double out_bytes_per_elem) const {
        return x3 ? s.gemm(cls, g, epi, out_bytes_per_elem) : s.weight_gemm(cls, g, epi, out_bytes_per_elem);
    }
    // LayerNorm of the stream into `act` (the layers' LayerNorms without the fold)
    int layer_norm(size_t gamma_off, size_t beta_off) const {
        LnExtra ex;
        ex.ldy = kx * Kp;  // normalised rows are K operands: row stride = E rounded up to the 64-wide K tile
        ex.x3 = x3;
        if (esm1) ex.eps = 1e-12f;  // ESM1LayerNorm (modules.py:44-65)
        return s.lnorm(x, gamma_off, beta_off, act, nullptr, N, ex);
    }
    // fold: a residual GEMM that also emits the next GEMM's rows and their statistics, and the pass that finishes those
    void producer(GemmArgs& a) const {
        a.h16 = act;
        a.ldh = Kp;
        a.ln_part = ln_part;
        a.ln_parts = w.ln_parts;
        a.ln_mean = ln_mean;
    }
    int finalize() const {
        ProfScope ps(m, s.st, PC_LN_STATS, 4.0 * N * w.ln_parts, (double)N * (8.0 * w.ln_parts + 12));
        ESMK_TRY(launch_ln_finalize(ln_part, ln_mean, ln_rstd, N, w.ln_parts, E, s.st));
        return 0;
    }
};

// the token-packed entries while the handle holds stream edits (esmk_set_stream_edits)
int refuse_edits_packed(const std::string& who, const esmk_model* m) {
    if (m->edits.empty()) return 0;
    return fail(who + ": stream edits are set (esmk_set_stream_edits): they run on padded batches only (esmk_forward, "
                      "esmk_forward_rows, esmk_forward_rows_contacts), a token-packed row space is not the caller's B*T rows");
}

// everything that needs no HIP call; the workspace plan
int check_forward(const ForwardCall& c, Workspace* w) {
    const std::string who(c.who);
    const esmk_model* m = c.m;
    if (!m || !c.packed || !c.tokens || !c.workspace) return fail(who + ": null argument");
    if (m->is_msa) return fail(who + ": MSA handle (use esmk_msa_forward)");
    if (c.pc && refuse_edits_packed(who, m)) return 1;
    if (c.B <= 0 || c.T <= 0) return fail(who + ": B and T must be positive");
    if ((long long)c.B * c.T > ESMK_MAX_ROWS) return fail(who + ": B*T exceeds 2^24 rows");
    if (c.n_repr > 0 && (!c.repr_layers || !c.repr_out)) return fail(who + ": null repr arrays");
    const bool want_attn = c.flags & ESMK_OUT_ATTN, want_contacts = c.flags & ESMK_OUT_CONTACTS;
    if ((c.flags & ESMK_OUT_ATTN_LOWP) && want_attn && want_contacts)
        return fail(who + ": ESMK_OUT_ATTN_LOWP cannot be combined with contacts computed from the attention tensor");
    if ((c.flags & ESMK_OUT_LOGITS) && !c.logits) return fail(who + ": logits buffer missing");
    if (want_attn && !c.attn) return fail(who + ": attention buffer missing");
    if (want_contacts && !c.contacts) return fail(who + ": contacts buffer missing");
    for (int i = 0; i < c.n_repr; ++i)
        if (c.repr_layers[i] < 0 || c.repr_layers[i] > m->L || !c.repr_out[i]) return fail(who + ": bad repr layer request");
    if (m->layer_limit > 0) {  // early exit: nothing above the last layer that runs can be asked for
        const std::string lim = ": a layer limit of " + std::to_string(m->layer_limit) + " is set (esmk_set_layer_limit): ";
        if (c.rs || c.ps || (c.pc && c.pc->maps)) return fail(who + lim + "this entry needs the whole stack");
        if (c.flags & ESMK_OUT_LOGITS) return fail(who + lim + "ESMK_OUT_LOGITS needs the whole stack");
        if (c.flags & (ESMK_OUT_ATTN | ESMK_OUT_ATTN_LOWP)) return fail(who + lim + "ESMK_OUT_ATTN / ESMK_OUT_ATTN_LOWP need the whole stack");
        if (c.flags & ESMK_OUT_CONTACTS) return fail(who + lim + "ESMK_OUT_CONTACTS needs the whole stack");
        for (int i = 0; i < c.n_repr; ++i)
            if (c.repr_layers[i] > m->layer_limit)
                return fail(who + lim + "representation " + std::to_string(c.repr_layers[i]) + " is above it");
        for (const esmk_stream_edit& e : m->edits)
            if (e.layer > m->layer_limit) return fail(who + lim + "a stream edit at layer " + std::to_string(e.layer) + " is above it");
    }
    *w = plan_workspace(m, c.B, c.T, c.flags, c.pc ? c.pc->n_seg : 0, c.pc ? c.pc->ct : nullptr, c.pc && c.pc->maps, c.ct_G);
    if (c.workspace_bytes < w->total) return fail(who + ": workspace too small");
    return 0;
}

// sinusoidal (ESM-1), rotary or unit tables for the longest run of positions
int position_tables(const Fwd& f) {
    esmk_model* m = f.m;
    if (f.esm1 && f.pc) return fail(f.who() + ": ESM-1 (no_rope = ESMK_ESM1) has no token-packed form yet");
    if (f.esm1 && ensure_sinus(m, f.T, f.s.st)) return 1;
    const int T_rope = f.pc ? f.pc->max_len : f.T;
    return m->cfg.no_rope ? ensure_unit_rope(m, T_rope, f.s.st) : ensure_rope(m, T_rope, f.s.st);
}

// token-packed batch: segment table, <pad> counts, the attention work list and, if asked for, the contact tables and the
// map offsets go behind the workspace in one upload (packed_tables: the layout)
int upload_packed_tables(Fwd& f) {
    esmk_model* m = f.m;
    const PackedCtx& pc = *f.pc;
    // with contacts the work list keeps the slots plan_workspace bounded it by: the contact tables do not move with n_items
    const PackedTables t = packed_tables(pc.n_seg, pc.ct ? packed_items_bound(pc.n_seg, f.T) : (size_t)pc.n_items,
                                         pc.ct ? pc.ct->table_ints() : 0, f.packed_maps);
    int* tab = f.at<int>(f.w.tables);
    if (m->pk_event) ESMK_TRY(hipEventSynchronize(m->pk_event));  // the previous upload has read the staging
    else ESMK_TRY(hipEventCreateWithFlags(&m->pk_event, hipEventDisableTiming));
    if (m->pk_host_cap < t.ints) {
        if (m->pk_host) ESMK_TRY(hipHostFree(m->pk_host));
        m->pk_host = nullptr;
        m->pk_host_cap = 0;
        ESMK_TRY(hipHostMalloc((void**)&m->pk_host, 2 * t.ints * 4, hipHostMallocDefault));
        m->pk_host_cap = 2 * t.ints;
    }
    int32_t* hostv = m->pk_host;
    if (f.packed_maps) hostv[t.map_base - 1] = 0;  // the alignment slot, if there is one: else a list below overwrites it
    fill_attn_tables(pc.seg_host, pc.n_seg, hostv);
    if (pc.ct) {  // contact offsets and work lists: the same upload
        contacts_packed_tables(*pc.ct, pc.seg_host, m->cfg.prepend_bos ? 1 : 0, m->cfg.append_eos ? 1 : 0, m->H, hostv + t.ct_base);
        f.ctd.seg = tab;
        f.ctd.off = reinterpret_cast<const long long*>(tab + t.ct_base);
        f.ctd.acc_work = tab + t.ct_base + 8 * (size_t)pc.n_seg;
        f.ctd.red_work = f.ctd.acc_work + 4 * pc.ct->n_acc;
        f.ctd.rt_work = f.ctd.red_work + 2 * pc.ct->n_red;
        f.ctd.fin_work = f.ctd.rt_work + pc.ct->n_rt;
        f.ctd.rows = f.T;
    }
    if (f.packed_maps) {
        fill_map_offsets(pc.seg_host, pc.n_seg, hostv + t.map_base);
        f.map_off = reinterpret_cast<const unsigned long long*>(tab + t.map_base);
    }
    ESMK_TRY(hipMemcpyAsync(tab, hostv, t.ints * 4, hipMemcpyHostToDevice, f.s.st));
    ESMK_TRY(hipEventRecord(m->pk_event, f.s.st));
    f.row_pos = f.at<int>(f.w.row_pos);
    f.segs.npad = tab + t.npad;
    f.segs.work = tab + t.work;
    return 0;
}

// the forms that run on some batches or some packed images only
int check_forms(const Fwd& f) {
    const esmk_model* m = f.m;
    if (f.x3 && (f.pc != nullptr || m->D != 64 || f.Kp != f.E || f.EA != f.E))
        return fail(f.who() + ": the f16x3 precision mode runs padded batches of head_dim-64 models (no token-packed form)");
    if (f.fold && m->fold_image != f.c.packed)
        return fail(f.who() + ": LayerNorm fold: this packed image is not the one the handle's weights were last packed "
                              "into (one image per handle at a time: re-pack, or use a second handle)");
    if (f.fold)
        for (int l = 0; l < f.L; ++l)
            if ((m->fold_state[l] & FB_ALL_W) != FB_ALL_W)
                return fail(f.who() + ": LayerNorm fold: the q/k/v or fc1 weights of layer " + std::to_string(l) +
                            " were not packed after the layer's LayerNorm parameters");
    return 0;
}

// esm2.py:82-98: token statistics, embedding (token dropout), positions of ESM-1 / ESM-1b
int embed_stage(const Fwd& f) {
    const esmk_model* m = f.m;
    const esmk_config& cfg = m->cfg;
    const PackedCtx* pc = f.pc;
    hipStream_t st = f.s.st;
    const int B = f.B, T = f.T, E = f.E;
    // pad columns [E, Kp) of the activation rows must be finite (they meet zero weight columns)
    if (f.Kp != E) {
        ESMK_TRY(hipMemsetAsync(f.h, 0, (size_t)f.N * std::max(f.Kp, f.EA) * f.s.os, st));
        if (f.fold) ESMK_TRY(hipMemsetAsync(f.ctx, 0, (size_t)f.N * std::max(f.Kp, f.EA) * f.s.os, st));
    }
    {
        ProfScope ps(f.m, st, PC_EMBED, 0, (double)f.N * 8 + 4.0 * f.N * E);
        const bool esm1b = cfg.num_positions > 0;
        const float* tok_emb = f.param(m->embed_f32);
        const int* tab = pc ? f.at<int>(f.w.tables) : nullptr;
        float* keep = esm1b ? f.at<float>(f.w.keep) : nullptr;
        if (f.esm1) {  // esm1.py:123-133: sqrt(E) x embedding, token dropout, + sinusoidal positions; no pad zeroing
            ESMK_TRY(launch_seq_stats(f.c.tokens, B, T, cfg.pad_idx, cfg.mask_idx, cfg.token_dropout, f.scale, f.key_bias, f.seq_info,
                                      st, nullptr));
            ESMK_TRY(launch_embed_esm1(f.c.tokens, tok_emb, f.scale, m->d_sinus, f.x, B, T, E, m->V, cfg.pad_idx, cfg.mask_idx,
                                       cfg.token_dropout, (float)sqrt((double)E), st));
        } else if (pc) {
            ESMK_TRY(launch_packed_stats(f.c.tokens, tab, pc->n_seg, T, cfg.pad_idx, cfg.mask_idx, f.scale, f.key_bias, f.row_pos,
                                         (int*)f.segs.npad, st, keep));
            // the token-dropout divisor is per row: "sequences" of one token
            ESMK_TRY(launch_embed(f.c.tokens, tok_emb, f.scale, f.x, T, 1, E, m->V, cfg.pad_idx, cfg.mask_idx, cfg.token_dropout, st));
        } else {
            ESMK_TRY(launch_seq_stats(f.c.tokens, B, T, cfg.pad_idx, cfg.mask_idx, cfg.token_dropout, f.scale, f.key_bias, f.seq_info,
                                      st, keep));
            ESMK_TRY(launch_embed(f.c.tokens, tok_emb, f.scale, f.x, B, T, E, m->V, cfg.pad_idx, cfg.mask_idx, cfg.token_dropout, st));
        }
        if (esm1b) {
            // esm1.py:133-139: + learned positions, emb_layer_norm_before, padded positions zeroed
            if ((pc ? pc->max_len : T) > cfg.num_positions - cfg.pad_idx - 1)
                return fail(f.who() + ": sequence length above the maximum of the positional embedding");
            if (pc)
                ESMK_TRY(launch_add_positions(f.c.tokens, f.param(m->pos_emb), f.x, pc->n_seg, pc->max_len, E, cfg.pad_idx,
                                              cfg.num_positions, st, tab));
            else
                ESMK_TRY(launch_add_positions(f.c.tokens, f.param(m->pos_emb), f.x, B, T, E, cfg.pad_idx, cfg.num_positions, st));
            if (cfg.ln_before) {
                LnExtra ex;
                ex.row_keep = keep;
                ESMK_TRY(launch_layernorm_ex(f.x, f.param(m->lnb_g), f.param(m->lnb_b), nullptr, f.x, f.N, E, f.s.op, ex, st));
            } else {
                ESMK_TRY(launch_scale_rows(f.x, keep, f.N, E, st));
            }
        }
    }
    return 0;
}

// The handle's edits of the stream after k layers (esmk_set_stream_edits), in list order: between the stage that wrote the
// stream and the capture of representation k.  With the fold the rows of layers 1 .. L-1 re-enter the chain here (operand
// row, mean, rstd by rowstats' arithmetic); for k = 0 the chain's entry pass follows, for k = L nothing reads the chain; the
// plain and split-weight modes have no chain state: their next LayerNorm pass reads x.
int stream_edit_stage(const Fwd& f, int k) {
    if (f.m->edits.empty()) return 0;
    const bool chain = f.fold && k >= 1 && k <= f.L - 1;
    for (const esmk_stream_edit& e : f.m->edits) {
        if (e.layer != k) continue;
        StreamEditArgs a = stream_edit_args(e, f.x, f.c.tokens, f.N, f.E);
        if (chain) {
            a.y = f.act;
            a.ldy = f.Kp;
            a.mean = f.ln_mean;
            a.rstd = f.ln_rstd;
        }
        const double rows = e.rows_dev ? (double)e.n_rows : (double)f.N;  // (an upper bound under the token selector)
        ProfScope ps(f.m, f.s.st, PC_STREAM_EDIT, 3.0 * rows * f.E, rows * f.E * ((e.src_dev ? 12.0 : 8.0) + (chain ? f.s.os : 0)));
        ESMK_TRY(launch_stream_edit(a, f.s.op, f.s.st));
    }
    return 0;
}

// self_attn_layer_norm and the q / k / v projections with RoPE (modules.py:123-124, multihead_attention.py:256-300)
int qkv_stage(const Fwd& f, const LayerOff& o, int l) {
    const esmk_model* m = f.m;
    hipStream_t st = f.s.st;
    const size_t os = f.s.os;
    // keys in [T,Tp) of V^T get probability exactly 0 but must be finite; the region is
    // shared with the FFN intermediate, so it is cleared every layer (odd T only).
    if (f.pc)  // only the spare key tile: every row below it is a computed (finite) row
        ESMK_TRY(hipMemset2DAsync((char*)f.vt + (size_t)f.T * os, (size_t)f.w.Tp * os, 0, 64 * os, (size_t)f.EA, st));
    else if (f.w.Tp != f.T) ESMK_TRY(hipMemsetAsync(f.vt, 0, (size_t)f.B * f.EA * f.w.Tp * os, st));
    if (!f.fold) {
        if (f.layer_norm(o.ln1g, o.ln1b)) return 1;
    } else if (l == 0) {  // entry of the fold chain: rows and statistics of the embedded stream
        ProfScope ps(f.m, st, PC_LN_STATS, 8.0 * f.N * f.E, (double)f.N * f.E * (4 + os));
        ESMK_TRY(launch_rowstats(f.x, f.act, f.ln_mean, f.ln_rstd, f.N, f.E, f.Kp, f.s.op, st));
    }
    QkvProj p;
    p.A = f.act;
    p.K = f.kx * f.Kp;
    p.W = f.s.pk + o.wqkv;
    p.split = split_plan(m).qk;
    p.bias = f.param(o.bqkv);
    if (f.fold) {
        p.ln_rstd = f.ln_rstd;
        p.bias2 = f.param(o.bqkv2);
    }
    p.q = f.q, p.k = f.k, p.vt = f.vt;
    p.cos = m->cfg.no_rope ? m->d_ucos : m->d_cos;
    p.sin = m->cfg.no_rope ? m->d_usin : m->d_sin;
    p.rows = f.N, p.T = f.T, p.Tp = f.w.Tp;
    // q carries d^-1/2 (multihead_attention.py:256-261) AND log2(e): the attention / map / contact kernels
    // work on log2-domain scores (softmax as exp2, see attention.hip)
    p.scaling = kLog2e / sqrtf((float)m->D);
    p.row_pos = f.row_pos;
    GemmArgs g, gv;
    qkv_gemm_args(m, p, &g, &gv);
    if (m->cfg.weight_split == 0 && gemm_qkv_one_launch(g)) {
        // small batches: q, k and v in one launch — same tiles, same bits, fewer rounds over the CUs (kernels.h, EPI_QKV_ALL)
        g.N = 3 * f.EA;
        return f.s.gemm(PC_GEMM_QKV, g, EPI_QKV_ALL, os);
    }
    if (f.layer_gemm(PC_GEMM_QKV, g, EPI_QKV_ROPE, os)) return 1;
    return f.layer_gemm(PC_GEMM_QKV, gv, EPI_V_T, os);
}

// the attention core (multihead_attention.py:318-394) into `ctx`, and what leaves the layer's q, k and row log-sum-exp
// while they are in the workspace: fused contact accumulation, attention maps
int attention_stage(const Fwd& f, const LayerOff& o, int l) {
    const esmk_model* m = f.m;
    const esmk_config& cfg = m->cfg;
    const PackedCtx* pc = f.pc;
    hipStream_t st = f.s.st;
    const int B = f.B, T = f.T, H = f.H, L = f.L, E = f.E, N = f.N, Tp = f.w.Tp, op = f.s.op;
    const size_t os = f.s.os;
    const double NE = (double)N * E;
    const bool d128 = m->D == 128;
    const float* ct_w = f.param(m->ct_w);
    {
        // 4 T d flop per (query, head) pair: QK^T and PV; q,k,v read + ctx written
        ProfScope ps(f.m, st, PC_ATTENTION, pc ? 4.0 * pc->sum_len2 * E : 4.0 * N * (double)T * E, 4 * NE * os);
        if (pc)  // gap rows of the context (the rows of h were last read by the two GEMMs above)
            ESMK_TRY(launch_zero_gap_rows(f.ctx, f.at<int>(f.w.tables), pc->n_seg, T, (size_t)f.EA * os, st));
        if (pc && d128)
            ESMK_TRY(launch_attention128_packed(f.q, f.k, f.vt, f.key_bias, f.ctx, f.lse, H, T, Tp, f.segs, pc->n_items, op, st));
        else if (pc) ESMK_TRY(launch_attention_packed(f.q, f.k, f.vt, f.key_bias, f.ctx, f.lse, H, T, Tp, f.segs, pc->n_items, op, st));
        else if (d128) ESMK_TRY(launch_attention128(f.q, f.k, f.vt, f.key_bias, f.seq_info, f.ctx, f.lse, B, H, T, Tp, op, st));
        else if (f.x3) ESMK_TRY(launch_attention_x3(f.q, f.k, f.vt, f.key_bias, f.seq_info, f.ctx, f.lse, B, H, T, Tp, op, st));
        else if (f.esm1)  // T + 1 keys: the learned null key / value pair of the layer (attention.hip, NK)
            ESMK_TRY(launch_attention_biaskv(f.q, f.k, f.vt, f.key_bias, f.seq_info, f.s.pk + o.bkv, f.s.pk + o.bkv + (size_t)f.EA * os,
                                             f.ctx, f.lse, B, H, T, Tp, op, st));
        else ESMK_TRY(launch_attention(f.q, f.k, f.vt, f.key_bias, f.seq_info, f.ctx, f.lse, B, H, T, Tp, op, st));
    }
    if (f.fused_ct && pc) {  // per segment (its [len,len] accumulators; segments with S <= 0 have no work)
        const CtPackedPlan& cp = *pc->ct;
        ProfScope ps(f.m, st, PC_ATTN_PROBS, 2.0 * cp.sum_len2 * E, 2 * NE * os + 8.0 * cp.sum_len2);
        ESMK_TRY(launch_contacts_packed_layer(f.q, f.k, f.lse, f.key_bias, f.c.tokens, ct_w, f.at<float>(f.w.ct_acc),
                                              f.at<float>(f.w.ct_row), f.at<float>(f.w.ct_col), f.at<float>(f.w.ct_rowp),
                                              f.at<float>(f.w.ct_colp), cp, f.ctd, H, L * H, l, head_slots(m), cfg.pad_idx,
                                              cfg.eos_idx, cfg.prepend_bos, cfg.append_eos, op, st));
    } else if (f.fused_ct && f.S_ct > 0) {
        // add the layer's channels to the [B,T,T] accumulator and the per-channel masked row / column sums
        ProfScope ps(f.m, st, PC_ATTN_PROBS, 2.0 * N * (double)T * E, 2 * NE * os + 8.0 * N * T);
        ESMK_TRY(launch_contacts_fused_layer(f.q, f.k, f.lse, f.key_bias, f.c.tokens, ct_w, f.at<float>(f.w.ct_acc),
                                             f.at<float>(f.w.ct_row), f.at<float>(f.w.ct_col), f.at<float>(f.w.ct_rowp),
                                             f.at<float>(f.w.ct_colp), B, H, T, L * H, l, head_slots(m), cfg.pad_idx, cfg.eos_idx,
                                             cfg.prepend_bos, cfg.append_eos, op, st, f.c.ct_G));
    }
    if (f.packed_maps) {  // multihead_attention.py:396-403 per segment: [L, H, len, len] blocks, no padding anywhere
        ProfScope ps(f.m, st, PC_ATTN_PROBS, 2.0 * pc->sum_len2 * E, 2 * NE * os + (pc->maps_lowp ? (double)os : 4.0) * pc->sum_len2 * H);
        if (d128)
            ESMK_TRY(launch_attention_probs128_packed(f.q, f.k, f.lse, f.key_bias, pc->maps_out, H, T, l, L, f.segs, f.map_off,
                                                      pc->n_items, op, pc->maps_lowp, st));
        else
            ESMK_TRY(launch_attention_probs_packed(f.q, f.k, f.lse, f.key_bias, pc->maps_out, H, T, l, L, f.segs, f.map_off,
                                                   pc->n_items, op, pc->maps_lowp, st));
    }
    if (f.want_attn) {
        ProfScope ps(f.m, st, PC_ATTN_PROBS, 2.0 * N * (double)T * E, 2 * NE * os + 4.0 * N * T * H);
        if (d128) ESMK_TRY(launch_attention_probs128(f.q, f.k, f.lse, f.key_bias, (float*)f.c.attn, B, H, T, l, L, op, st, f.attn_lowp));
        else ESMK_TRY(launch_attention_probs(f.q, f.k, f.lse, f.key_bias, (float*)f.c.attn, B, H, T, l, L, op, st, f.attn_lowp));
    }
    return 0;
}

// x += out_proj(context) (modules.py:125-133), then final_layer_norm (modules.py:135-136) — with the fold as statistics of
// the rows the residual epilogue wrote
int out_proj_stage(const Fwd& f, const LayerOff& o) {
    GemmArgs g;
    g.A = f.ctx;
    g.W = f.s.pk + o.wo;
    g.bias = f.param(o.bo);
    g.out = f.x;
    g.M = f.N;
    g.N = f.E;
    g.K = f.kx * f.EA;
    if (f.fold) f.producer(g);
    if (f.layer_gemm(PC_GEMM_OUT, g, EPI_RESID_F32, f.fold ? 8 + f.s.os : 8)) return 1;
    return f.fold ? f.finalize() : f.layer_norm(o.ln2g, o.ln2b);
}

// x += fc2(gelu(fc1(.))) (modules.py:137-140)
int ffn_stage(const Fwd& f, const LayerOff& o, int l) {
    GemmArgs g;
    g.A = f.act;
    g.W = f.s.pk + o.w1;
    g.bias = f.param(o.b1);
    if (f.fold) {
        g.ln_rstd = f.ln_rstd;
        g.bias2 = f.param(o.b12);
    }
    g.out = f.ffn;
    g.M = f.N;
    g.N = f.F;
    g.K = f.kx * f.Kp;
    g.x3_out = f.x3;  // fc1 + GELU writing the hi | hi | lo rows of fc2's operand
    if (f.layer_gemm(PC_GEMM_FC1, g, EPI_GELU_T, f.kx * f.s.os)) return 1;
    g = GemmArgs();
    g.A = f.ffn;
    g.W = f.s.pk + o.w2;
    g.bias = f.param(o.b2);
    g.out = f.x;
    g.M = f.N;
    g.N = f.E;
    g.K = f.kx * f.F;
    const bool feeds_next = f.fold && l + 1 < f.L;  // the next layer's q/k/v projections read the rows this GEMM writes
    if (feeds_next) f.producer(g);
    if (f.layer_gemm(PC_GEMM_FC2, g, EPI_RESID_F32, feeds_next ? 8 + f.s.os : 8)) return 1;
    return feeds_next ? f.finalize() : 0;
}

// The head of the model runs on the rows it is asked for: all N of them, or (esmk_forward_rows) the selection gathered
// out of the final stream.  Every kernel below computes a row from that row alone, so a selected row carries the bits
// the same row has in esmk_forward.
int head_stage(const Fwd& f) {
    const esmk_model* m = f.m;
    const RowSel* rs = f.c.rs;
    const Stack& s = f.s;
    const int E = f.E, Kp = f.Kp;
    int rows = f.N;
    float *x = f.x, *g32 = f.g32;
    void* h = f.h;
    if (rs && rs->n_sel == 0) return 0;  // esmk_forward_rows_contacts with no rows selected: no head runs
    if (rs) {
        rows = rs->n_sel;
        x = f.at<float>(rs->x);
        h = f.ws + rs->h;
        g32 = f.at<float>(rs->g32);
        ProfScope ps(f.m, s.st, PC_COPY, 0, 8.0 * rows * E);
        ESMK_TRY(launch_gather_rows(f.x, rs->sel_dev, x, f.N, E, rows, s.st));
        if (Kp != E) ESMK_TRY(hipMemsetAsync(h, 0, (size_t)rows * std::max(Kp, f.EA) * s.os, s.st));  // finite pad columns
    }
    if (f.esm1) {
        // esm1.py:173-175: no final LayerNorm; logits = x . embed_out^T (+ embed_out_bias): one GEMM on the rounded stream
        if (f.want_logits) {
            {
                ProfScope ps(f.m, s.st, PC_COPY, 0, (4 + s.os) * (double)rows * E);
                ESMK_TRY(launch_convert(x, ESMK_DT_F32, h, s.op, (size_t)rows * E, s.st));  // head_dim 64: Kp == E
            }
            GemmArgs g;
            g.A = h;
            g.W = s.pk + m->out_w;
            g.bias = m->final_bias ? f.param(m->out_b) : nullptr;
            g.out = f.c.logits;
            g.M = rows;
            g.N = m->V;
            g.K = Kp;
            if (s.gemm(PC_LM_LOGITS, g, EPI_STORE_F32, 4)) return 1;
        }
    } else {
        LnExtra ex;
        ex.ldy = Kp;
        void* rep_lp = s.repr_of(f.L);
        if (f.repr_lowp && rep_lp != nullptr) {
            // representation L in the operand dtype: the normalised rows h ARE that tensor when their row stride is E
            if (Kp == E) {
                if (s.lnorm(x, m->fin_g, m->fin_b, f.want_logits ? h : rep_lp, nullptr, rows, ex)) return 1;
                if (f.want_logits) ESMK_TRY(hipMemcpyAsync(rep_lp, h, (size_t)f.N * E * s.os, hipMemcpyDeviceToDevice, s.st));
            } else {  // padded row stride (E = 480): through the fp32 scratch
                if (s.lnorm(x, m->fin_g, m->fin_b, f.want_logits ? h : nullptr, g32, rows, ex)) return 1;
                ESMK_TRY(launch_convert(g32, ESMK_DT_F32, rep_lp, s.op, (size_t)f.N * E, s.st));
            }
            for (int i = 0; i < s.n_repr; ++i)  // duplicates of layer L, if any
                if (s.repr_layers[i] == f.L && s.repr_out[i] != rep_lp)
                    ESMK_TRY(hipMemcpyAsync(s.repr_out[i], rep_lp, (size_t)f.N * E * s.os, hipMemcpyDeviceToDevice, s.st));
        }
        if (lm_head(s, rows, x, h, g32, Kp, ex, f.repr_lowp, f.want_logits, f.c.logits)) return 1;
    }
    if (rs) {  // torch.log_softmax(logits, dim=-1) of the selected rows.  Profiles of this entry have no classes of their own:
        // the log-softmax is counted under "lm_head_logits", the gather (and its pad-column memset) under "repr_copy"
        ProfScope ps(f.m, s.st, PC_LM_LOGITS, 0, 8.0 * rows * m->V);
        ESMK_TRY(launch_log_softmax_rows((const float*)f.c.logits, rs->logprobs_out, nullptr, nullptr, rows, m->V, s.st));
    }
    return 0;
}

// contacts from what the layers accumulated (fused), or from the attention tensor (esm2.py:140-142)
int contacts_final(const Fwd& f) {
    const esmk_model* m = f.m;
    const esmk_config& cfg = m->cfg;
    hipStream_t st = f.s.st;
    const int B = f.B, T = f.T, H = f.H, L = f.L;
    const float *ct_w = f.param(m->ct_w), *ct_b = f.param(m->ct_b);
    if (f.fused_ct && f.pc) {
        const CtPackedPlan& cp = *f.pc->ct;
        ProfScope ps(f.m, st, PC_CONTACTS, 0, 4.0 * ((double)cp.sum_len2 * 2 + 3.0 * L * H * T));
        ESMK_TRY(launch_contacts_packed_final(f.at<float>(f.w.ct_acc), f.at<float>(f.w.ct_row), f.at<float>(f.w.ct_col),
                                              f.at<float>(f.w.ct_wt), f.c.tokens, ct_w, ct_b, (float*)f.c.contacts, cp, f.ctd, L * H,
                                              cfg.pad_idx, cfg.eos_idx, cfg.prepend_bos, cfg.append_eos, st));
    } else if (f.fused_ct && f.S_ct > 0) {
        ProfScope ps(f.m, st, PC_CONTACTS, 0, 4.0 * B * ((double)T * T * 2 + 3.0 * L * H * T));
        ESMK_TRY(launch_contacts_fused_final(f.at<float>(f.w.ct_acc), f.at<float>(f.w.ct_row), f.at<float>(f.w.ct_col),
                                             f.at<float>(f.w.ct_wt), f.c.tokens, ct_w, ct_b, (float*)f.c.contacts, B, H, L * H, T,
                                             head_slots(m), cfg.pad_idx, cfg.eos_idx, cfg.prepend_bos, cfg.append_eos, st,
                                             f.c.ct_G));
    } else if (f.want_contacts && f.S_ct > 0) {
        // (an empty sequence has an empty [B,0,0] contact map: nothing to compute)
        ProfScope ps(f.m, st, PC_CONTACTS, 0, 2.0 * 4 * B * (double)L * H * T * T);
        ESMK_TRY(launch_contacts((const float*)f.c.attn, f.c.tokens, ct_w, ct_b, f.at<float>(f.w.ct_scratch), (float*)f.c.contacts,
                                 B, L * H, T, cfg.eos_idx, cfg.prepend_bos, cfg.append_eos, st));
    }
    return 0;
}

// the handle's pairwise head (esmk_set_pair_head) on the stashed q / k / lse of every layer: all L*H channels in one launch
int pair_head_final(const Fwd& f) {
    const esmk_model* m = f.m;
    const esmk_config& cfg = m->cfg;
    const PairStash& ps = *f.c.ps;
    const int C_out = m->pair_sym + m->pair_asym;
    const double pairs = (double)f.B * f.S_ct * f.S_ct;
    ProfScope scope(f.m, f.s.st, PC_CONTACTS, 2.0 * pairs * f.L * f.H * C_out,
                    2.0 * f.L * (double)ps.qk_layer + 3.0 * 4 * pairs * C_out);
    ESMK_TRY(launch_pair_head(f.ws + ps.q, f.ws + ps.k, (const float*)(f.ws + ps.lse), f.key_bias, f.c.tokens, m->d_pair_w64,
                              m->d_pair_bias, ps.out, f.L, f.B, f.H, f.T, head_slots(m), m->pair_sym, m->pair_asym, cfg.pad_idx,
                              cfg.prepend_bos, cfg.append_eos, f.s.op, f.s.st));
    return 0;
}

int forward_impl(const ForwardCall& c) {
    Workspace w;
    if (check_forward(c, &w)) return 1;
    Fwd f(c, w);
    if (position_tables(f)) return 1;
    if (f.pc && upload_packed_tables(f)) return 1;
    if (check_forms(f)) return 1;
    if (embed_stage(f)) return 1;
    if (stream_edit_stage(f, 0)) return 1;
    if (f.s.repr_copy(0, f.x, f.repr_lowp)) return 1;  // esm2.py:99-100
    // early exit (esmk_set_layer_limit): the stack ends after `layers` layers; with the fold the last residual epilogue still
    // emits the next layer's operand rows, which nothing reads
    const int layers = f.m->layer_limit > 0 ? f.m->layer_limit : f.L;
    for (int l = 0; l < layers; ++l) {  // esm2.py:111-121 -> modules.py:120-142
        const LayerOff& o = f.m->layer[l];
        if (c.ps) {  // the layer's q, k and lse stay: slot l of the stash (pair_head.hip reads all of them after the last layer)
            f.q = f.ws + c.ps->q + (size_t)l * c.ps->qk_layer;
            f.k = f.ws + c.ps->k + (size_t)l * c.ps->qk_layer;
            f.lse = (float*)(f.ws + c.ps->lse + (size_t)l * c.ps->lse_layer);
        }
        if (qkv_stage(f, o, l)) return 1;        // self_attn_layer_norm; q, k, v
        if (attention_stage(f, o, l)) return 1;  // softmax(q k^T) v
        if (out_proj_stage(f, o)) return 1;      // x += out_proj(.); final_layer_norm
        if (ffn_stage(f, o, l)) return 1;        // x += fc2(gelu(fc1(.)))
        if (stream_edit_stage(f, l + 1)) return 1;
        // esm2.py:117-118; ESM-1: layer L too (no final LayerNorm)
        if ((l + 1 < f.L || f.esm1) && f.s.repr_copy(l + 1, f.x, f.repr_lowp)) return 1;
    }
    if (layers < f.L) return 0;  // (check_forward: no head, map or contact output is asked for under a limit)
    if (head_stage(f)) return 1;
    if (c.ps) return pair_head_final(f);
    return contacts_final(f);
}

}  // namespace

extern "C" {

const char* esmk_last_error(void) { return g_err.c_str(); }
#ifndef ESMK_SRC_HASH
#define ESMK_SRC_HASH "unhashed-build---"
#endif
// "esmk-src:" + the SHA-256 prefix of the sources (esm_amd/build.py: source_hash) — also read straight from the file
const char* esmk_version(void) { return "esmk 0.2 (gfx950) esmk-src:" ESMK_SRC_HASH; }

int esmk_create(const esmk_config* cfg, esmk_model** out) {
    if (!cfg || !out) return fail("esmk_create: null argument");
    if (cfg->num_layers <= 0 || cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->ffn_dim <= 0 ||
        cfg->vocab <= 0)
        return fail("esmk_create: non-positive dimension");
    if (cfg->embed_dim % cfg->num_heads != 0)
        return fail("esmk_create: embed_dim must be divisible by num_heads");
    if (cfg->operand_dtype != ESMK_F16 && cfg->operand_dtype != ESMK_BF16)
        return fail("esmk_create: operand_dtype must be ESMK_F16 or ESMK_BF16");
    const int d = cfg->embed_dim / cfg->num_heads;
    if ((d > 64 && d != 128) || d < 2 || (d & 1))
        return fail("esmk_create: head_dim " + std::to_string(d) +
                    " is not supported by the gfx950 attention kernels (128, or an even head_dim <= 64; smaller "
                    "heads are spread over 64 slots at pack time)");
    if (cfg->embed_dim % 8 != 0 || cfg->ffn_dim % 64 != 0)
        return fail("esmk_create: embed_dim must be a multiple of 8 and ffn_dim a multiple of 64");
    if (cfg->weight_split < 0 || cfg->weight_split > 4)
        return fail("esmk_create: weight_split must be 0 (off), 1 (f16x2), 2 (f16x2a), 3 (f16x2v) or 4 (f16x3)");
    if (cfg->weight_split == 4 && (cfg->embed_dim % 64 != 0 || cfg->embed_dim / cfg->num_heads != 64))
        return fail("esmk_create: weight_split 4 (f16x3) needs head_dim 64 and embed_dim % 64 == 0");
    if (cfg->weight_split != 0 && cfg->operand_dtype != ESMK_F16)
        return fail("esmk_create: weight_split (precision modes f16x2 / f16x2a / f16x2v / f16x3) needs operand_dtype ESMK_F16");
    if (cfg->no_rope < 0 || (cfg->no_rope > 1 && cfg->no_rope != ESMK_ESM1 && cfg->no_rope != (ESMK_ESM1 | ESMK_ESM1_FINAL_BIAS)))
        return fail("esmk_create: no_rope must be 0, 1, ESMK_ESM1 (2) or ESMK_ESM1 | ESMK_ESM1_FINAL_BIAS (6): final_bias belongs to ESM-1");
    const bool cfg_esm1 = (cfg->no_rope & ESMK_ESM1) != 0;
    if (cfg_esm1) {  // ESM-1 (protein_bert_base): what this family does not have is refused here, before any HIP call
        if (d != 64) return fail("esmk_create: ESM-1 (no_rope = ESMK_ESM1, bias_kv attention) needs head_dim 64, got " + std::to_string(d));
        if (cfg->weight_split != 0)
            return fail("esmk_create: ESM-1 (no_rope = ESMK_ESM1) runs with plain fp16 / bf16 operands only (weight_split must be 0)");
        if (cfg->ln_fold > 0)
            return fail("esmk_create: ESM-1 (no_rope = ESMK_ESM1) has no LayerNorm fold (LayerNorm eps 1e-12, no final LayerNorm): ln_fold "
                        "must be 0 or -1");
        if (cfg->num_positions != 0 || cfg->ln_before != 0)
            return fail("esmk_create: ESM-1 (no_rope = ESMK_ESM1) has sinusoidal positions and no embedding LayerNorm: num_positions and "
                        "ln_before must be 0");
    }
    // LayerNorm fold: explicit request, or the library default / ESMK_LN_FOLD where the configuration supports it
    const bool fold_ok = cfg->weight_split == 0 && d <= 64 && !cfg_esm1;
    if (cfg->ln_fold > 0 && !fold_ok)
        return fail("esmk_create: ln_fold needs plain fp16 / bf16 operands (no weight_split) and head_dim <= 64");
    bool fold = cfg->ln_fold > 0;
    if (cfg->ln_fold == 0 && fold_ok) {
        const char* e = getenv("ESMK_LN_FOLD");
        fold = e ? atoi(e) != 0 : kLnFoldDefault;
    }
    esmk_model* m = new esmk_model();
    m->fold = fold;
    m->fold_state.assign(cfg->num_layers, 0u);
    m->cfg = *cfg;
    m->esm1 = cfg_esm1 ? 1 : 0;
    m->final_bias = (cfg->no_rope & ESMK_ESM1_FINAL_BIAS) ? 1 : 0;
    m->L = cfg->num_layers;
    m->E = cfg->embed_dim;
    m->H = cfg->num_heads;
    m->F = cfg->ffn_dim;
    m->V = cfg->vocab;
    m->D = d;
    m->EA = m->H * head_slots(m);
    m->Kp = (m->E + 63) / 64 * 64;
    plan_packed(m);
    *out = m;
    return 0;
}

void esmk_destroy(esmk_model* m) {
    if (!m) return;
    if (m->d_cos) (void)hipFree(m->d_cos);
    if (m->d_sin) (void)hipFree(m->d_sin);
    if (m->d_inv_freq) (void)hipFree(m->d_inv_freq);
    if (m->d_ucos) (void)hipFree(m->d_ucos);
    if (m->d_usin) (void)hipFree(m->d_usin);
    if (m->d_sinus) (void)hipFree(m->d_sinus);
    if (m->pk_host) (void)hipHostFree(m->pk_host);
    if (m->d_pair_w64) (void)hipFree(m->d_pair_w64);
    if (m->d_pair_bias) (void)hipFree(m->d_pair_bias);
    if (m->pk_event) (void)hipEventDestroy(m->pk_event);
    delete m;
}

int esmk_set_rope_inv_freq(esmk_model* m, const float* inv_freq_host, int n) {
    if (!m || !inv_freq_host) return fail("esmk_set_rope_inv_freq: null argument");
    if (n != m->D / 2) return fail("esmk_set_rope_inv_freq: expected head_dim/2 values");
    // 32 slots (64 for head_dim 128): slot i < d/2 carries frequency i, the rest rotate by angle 0 (they only
    // ever see zeros)
    const int slots = m->D == 128 ? 64 : 32;
    m->inv_freq.assign(slots, 0.f);
    for (int i = 0; i < n; ++i) m->inv_freq[i] = inv_freq_host[i];
    if (!m->d_inv_freq) ESMK_TRY(hipMalloc(&m->d_inv_freq, (size_t)slots * 4));
    ESMK_TRY(hipMemcpy(m->d_inv_freq, m->inv_freq.data(), (size_t)slots * 4, hipMemcpyHostToDevice));
    m->rope_cap = 0;  // tables are rebuilt on the next forward
    return 0;
}

int esmk_packed_bytes(const esmk_model* m, size_t* bytes) {
    if (!m || !bytes) return fail("esmk_packed_bytes: null argument");
    *bytes = m->packed_bytes;
    return 0;
}

int esmk_pack_weight(esmk_model* m, void* packed_dev, size_t packed_bytes, const char* key,
                     const void* src_dev, int src_dtype, const int64_t* shape, int ndim,
                     void* stream) {
    if (!m || !packed_dev || !key || !src_dev) return fail("esmk_pack_weight: null argument");
    if (packed_bytes < m->packed_bytes) return fail("esmk_pack_weight: packed buffer too small");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)packed_dev;
    const int op = m->cfg.operand_dtype;
    const size_t os = op_size(op);
    const size_t E = m->E, F = m->F, V = m->V;
    const size_t n = numel(shape, ndim);
    auto put = [&](size_t off, int dst_dtype, size_t expect) -> int {
        if (n != expect)
            return fail(std::string("esmk_pack_weight: ") + key + " has " + std::to_string(n) +
                        " elements, expected " + std::to_string(expect));
        ESMK_TRY(launch_convert(src_dev, src_dtype, base + off, dst_dtype, n, st));
        return 0;
    };
    // [rows, cols] matrix into a destination with row stride ld; rmap / cmap spread head_dim-d heads over
    // 64 slots (elementwise.hip: head_pad_index).  The packed image is zero-initialised by the caller, so
    // padded rows / columns stay zero.
    const size_t EA = m->EA, Kp = m->Kp;
    const int hd = m->D;
    const int padmap = (hd < 64) ? 1 : 0;        // q, k, v, out_proj: heads spread over 64 slots
    const int qkmap = (hd != 64) ? 1 : 0;        // q, k additionally: slice order of 128-wide heads
    auto put2d = [&](size_t off, int dst_dtype, size_t rows, size_t cols, size_t ld, int rmap, int cmap) -> int {
        if (n != rows * cols)
            return fail(std::string("esmk_pack_weight: ") + key + " has " + std::to_string(n) +
                        " elements, expected " + std::to_string(rows * cols));
        ESMK_TRY(launch_convert2d(src_dev, src_dtype, base + off, dst_dtype, rows, cols, ld, rmap, cmap, hd, st));
        return 0;
    };
    // a matrix of the layer stack: plain operand-dtype image, or (f16x2) the hi | lo split image with rows of 2 ld
    const size_t ws = m->cfg.weight_split ? 2 : 1;
    const SplitPlan sp = split_plan(m);  // factor 2 = W_hi | W_lo image
    auto putw = [&](size_t off, size_t rows, size_t cols, size_t ld, int rmap, int cmap, size_t split = 0) -> int {
        if ((split ? split : ws) == 1) return put2d(off, op, rows, cols, ld, rmap, cmap);
        if (n != rows * cols)
            return fail(std::string("esmk_pack_weight: ") + key + " has " + std::to_string(n) +
                        " elements, expected " + std::to_string(rows * cols));
        ESMK_TRY(launch_convert2d_split(src_dev, src_dtype, base + off, rows, cols, ld, rmap, cmap, hd, st, (int)(split ? split : ws)));
        return 0;
    };
    if (!strcmp(key, "embed_tokens.weight")) {
        if (put(m->embed_f32, ESMK_DT_F32, V * E)) return 1;
        return put2d(m->embed_op, op, V, E, Kp, 0, 0);
    }
    if (m->is_msa) {
        if (!strcmp(key, "embed_positions.weight")) return put(m->pos_emb, ESMK_DT_F32, (size_t)m->npos * E);
        if (!strcmp(key, "msa_position_embedding")) return put(m->msa_pos, ESMK_DT_F32, (size_t)1024 * E);
        if (!strcmp(key, "emb_layer_norm_before.weight")) return put(m->lnb_g, ESMK_DT_F32, E);
        if (!strcmp(key, "emb_layer_norm_before.bias")) return put(m->lnb_b, ESMK_DT_F32, E);
        if (starts_with(key, "layers.")) {
            char* end = nullptr;
            const long l = strtol(key + 7, &end, 10);
            if (end == key + 7 || *end != '.' || l < 0 || l >= m->L)
                return fail(std::string("esmk_pack_weight: bad layer index in ") + key);
            const char* sub = end + 1;
            const MsaLayerOff& o = m->mlayer[l];
            const AttnOff* a = nullptr;
            if (starts_with(sub, "row_self_attention.")) { a = &o.row; sub += 19; }
            else if (starts_with(sub, "column_self_attention.")) { a = &o.col; sub += 22; }
            if (a) {
                if (!strcmp(sub, "layer.q_proj.weight")) return putw(a->wqkv, E, E, E, 0, 0, sp.qk);
                if (!strcmp(sub, "layer.k_proj.weight")) return putw(a->wqkv + E * E * os * sp.qk, E, E, E, 0, 0, sp.qk);
                if (!strcmp(sub, "layer.v_proj.weight")) return putw(a->wqkv + 2 * E * E * os * sp.qk, E, E, E, 0, 0, sp.v);
                if (!strcmp(sub, "layer.q_proj.bias")) return put(a->bqkv, ESMK_DT_F32, E);
                if (!strcmp(sub, "layer.k_proj.bias")) return put(a->bqkv + E * 4, ESMK_DT_F32, E);
                if (!strcmp(sub, "layer.v_proj.bias")) return put(a->bqkv + 2 * E * 4, ESMK_DT_F32, E);
                if (!strcmp(sub, "layer.out_proj.weight")) return putw(a->wo, E, E, E, 0, 0, sp.o);
                if (!strcmp(sub, "layer.out_proj.bias")) return put(a->bo, ESMK_DT_F32, E);
                if (!strcmp(sub, "layer_norm.weight")) return put(a->lng, ESMK_DT_F32, E);
                if (!strcmp(sub, "layer_norm.bias")) return put(a->lnb, ESMK_DT_F32, E);
                return 0;
            }
            if (!strcmp(sub, "feed_forward_layer.layer.fc1.weight")) return putw(o.w1, F, E, E, 0, 0, sp.ffn);
            if (!strcmp(sub, "feed_forward_layer.layer.fc1.bias")) return put(o.b1, ESMK_DT_F32, F);
            if (!strcmp(sub, "feed_forward_layer.layer.fc2.weight")) return putw(o.w2, E, F, F, 0, 0, sp.ffn);
            if (!strcmp(sub, "feed_forward_layer.layer.fc2.bias")) return put(o.b2, ESMK_DT_F32, E);
            if (!strcmp(sub, "feed_forward_layer.layer_norm.weight")) return put(o.flng, ESMK_DT_F32, E);
            if (!strcmp(sub, "feed_forward_layer.layer_norm.bias")) return put(o.flnb, ESMK_DT_F32, E);
            return 0;
        }
    }
    if (m->esm1) {  // ESM-1: untied output projection (esm1.py:111-114,174)
        if (!strcmp(key, "embed_out")) return put2d(m->out_w, op, V, E, Kp, 0, 0);
        if (!strcmp(key, "embed_out_bias")) {
            if (!m->final_bias) return fail("esmk_pack_weight: embed_out_bias on an ESM-1 handle created without final_bias");
            return put(m->out_b, ESMK_DT_F32, V);
        }
    }
    if (!strcmp(key, "lm_head.weight")) return 0;  // tied to embed_tokens.weight (esm2.py:71-75)
    if (!m->is_msa && m->cfg.num_positions > 0 && !strcmp(key, "embed_positions.weight"))
        return put(m->pos_emb, ESMK_DT_F32, (size_t)m->cfg.num_positions * E);
    if (!m->is_msa && m->cfg.ln_before && !strcmp(key, "emb_layer_norm_before.weight")) return put(m->lnb_g, ESMK_DT_F32, E);
    if (!m->is_msa && m->cfg.ln_before && !strcmp(key, "emb_layer_norm_before.bias")) return put(m->lnb_b, ESMK_DT_F32, E);
    if (!strcmp(key, "emb_layer_norm_after.weight")) return put(m->fin_g, ESMK_DT_F32, E);
    if (!strcmp(key, "emb_layer_norm_after.bias")) return put(m->fin_b, ESMK_DT_F32, E);
    if (!strcmp(key, "lm_head.dense.weight")) {
        if (m->cfg.weight_split && put(m->lm_w32, ESMK_DT_F32, E * E)) return 1;
        return put2d(m->lm_w, op, E, E, Kp, 0, 0);
    }
    if (!strcmp(key, "lm_head.dense.bias")) return put(m->lm_b, ESMK_DT_F32, E);
    if (!strcmp(key, "lm_head.layer_norm.weight")) return put(m->lm_lng, ESMK_DT_F32, E);
    if (!strcmp(key, "lm_head.layer_norm.bias")) return put(m->lm_lnb, ESMK_DT_F32, E);
    if (!strcmp(key, "lm_head.bias")) return put(m->lm_bias, ESMK_DT_F32, V);
    if (!strcmp(key, "contact_head.regression.weight"))
        return put(m->ct_w, ESMK_DT_F32, (size_t)m->L * m->H);
    if (!strcmp(key, "contact_head.regression.bias")) return put(m->ct_b, ESMK_DT_F32, 1);
    if (starts_with(key, "layers.")) {
        char* end = nullptr;
        const long l = strtol(key + 7, &end, 10);
        if (end == key + 7 || *end != '.' || l < 0 || l >= m->L)
            return fail(std::string("esmk_pack_weight: bad layer index in ") + key);
        const char* sub = end + 1;
        const LayerOff& o = m->layer[l];
        // LayerNorm fold: q/k/v and fc1 weights are packed as gamma-folded, row-centred images + W . beta (bias2); the
        // LayerNorm parameters they fold must be in the image already, and packing one of those later marks the folded
        // weights stale (esmk_forward refuses to run on a stale fold)
        if (m->fold && m->fold_image != packed_dev) {  // another image: its folds start unpacked
            m->fold_state.assign(m->L, 0u);
            m->fold_image = packed_dev;
        }
        uint32_t& fs = m->fold_state[l];
        // LayerNorm parameter of a fold: the "present" bit is set only once the copy was queued; the folded weights that
        // depend on it are stale from the moment the call is made, whether or not it succeeds
        auto ln_put = [&](size_t off, uint32_t present, uint32_t stale) -> int {
            fs &= ~(stale | present);
            if (put(off, ESMK_DT_F32, E)) return 1;
            fs |= present;
            return 0;
        };
        auto fold_put = [&](size_t woff, size_t b2off, size_t rows, int rmap, size_t lng, size_t lnb, uint32_t need,
                            uint32_t done) -> int {
            if ((fs & need) != need)
                return fail(std::string("esmk_pack_weight: ") + key + ": with the LayerNorm fold the layer's LayerNorm weight "
                            "and bias must be packed before its q/k/v and fc1 weights");
            if (n != rows * E)
                return fail(std::string("esmk_pack_weight: ") + key + " has " + std::to_string(n) + " elements, expected " +
                            std::to_string(rows * E));
            ESMK_TRY(launch_fold_weight(src_dev, src_dtype, (const float*)(base + lng), (const float*)(base + lnb), base + woff, op,
                                        (float*)(base + b2off), rows, E, Kp, rmap, hd, st));
            fs |= done;
            return 0;
        };
        if (m->fold) {
            if (!strcmp(sub, "self_attn.q_proj.weight")) return fold_put(o.wqkv, o.bqkv2, E, qkmap, o.ln1g, o.ln1b, FB_LN1G | FB_LN1B, FB_WQ);
            if (!strcmp(sub, "self_attn.k_proj.weight")) return fold_put(o.wqkv + EA * Kp * os, o.bqkv2 + EA * 4, E, qkmap, o.ln1g, o.ln1b, FB_LN1G | FB_LN1B, FB_WK);
            if (!strcmp(sub, "self_attn.v_proj.weight")) return fold_put(o.wqkv + 2 * EA * Kp * os, o.bqkv2 + 2 * EA * 4, E, padmap, o.ln1g, o.ln1b, FB_LN1G | FB_LN1B, FB_WV);
            if (!strcmp(sub, "fc1.weight")) return fold_put(o.w1, o.b12, F, 0, o.ln2g, o.ln2b, FB_LN2G | FB_LN2B, FB_W1);
            if (!strcmp(sub, "self_attn_layer_norm.weight")) return ln_put(o.ln1g, FB_LN1G, FB_WQ | FB_WK | FB_WV);
            if (!strcmp(sub, "self_attn_layer_norm.bias")) return ln_put(o.ln1b, FB_LN1B, FB_WQ | FB_WK | FB_WV);
            if (!strcmp(sub, "final_layer_norm.weight")) return ln_put(o.ln2g, FB_LN2G, FB_W1);
            if (!strcmp(sub, "final_layer_norm.bias")) return ln_put(o.ln2b, FB_LN2B, FB_W1);
        }
        // ESM-1: the null key / value rows [1,1,E] = [H,64] per head, operand dtype; bias_k is NOT scaled (only q carries the scale)
        if (m->esm1 && !strcmp(sub, "self_attn.bias_k")) return put(o.bkv, op, E);
        if (m->esm1 && !strcmp(sub, "self_attn.bias_v")) return put(o.bkv + EA * os, op, E);
        // q/k/v: output rows are head dims -> spread over 64 slots; input columns padded to Kp
        if (!strcmp(sub, "self_attn.q_proj.weight")) return putw(o.wqkv, E, E, Kp, qkmap, 0, sp.qk);
        if (!strcmp(sub, "self_attn.k_proj.weight")) return putw(o.wqkv + EA * Kp * os * sp.qk, E, E, Kp, qkmap, 0, sp.qk);
        if (!strcmp(sub, "self_attn.v_proj.weight")) return putw(o.wqkv + 2 * EA * Kp * os * sp.qk, E, E, Kp, padmap, 0, sp.v);
        if (!strcmp(sub, "self_attn.q_proj.bias")) return put2d(o.bqkv, ESMK_DT_F32, 1, E, EA, 0, qkmap);
        if (!strcmp(sub, "self_attn.k_proj.bias")) return put2d(o.bqkv + EA * 4, ESMK_DT_F32, 1, E, EA, 0, qkmap);
        if (!strcmp(sub, "self_attn.v_proj.bias")) return put2d(o.bqkv + 2 * EA * 4, ESMK_DT_F32, 1, E, EA, 0, padmap);
        // out_proj consumes the attention context: its input columns follow the same slot layout
        if (!strcmp(sub, "self_attn.out_proj.weight")) return putw(o.wo, E, E, EA, 0, padmap, sp.o);
        if (!strcmp(sub, "self_attn.out_proj.bias")) return put(o.bo, ESMK_DT_F32, E);
        if (!strcmp(sub, "fc1.weight")) return putw(o.w1, F, E, Kp, 0, 0, sp.ffn);
        if (!strcmp(sub, "fc1.bias")) return put(o.b1, ESMK_DT_F32, F);
        if (!strcmp(sub, "fc2.weight")) return putw(o.w2, E, F, F, 0, 0, sp.ffn);
        if (!strcmp(sub, "fc2.bias")) return put(o.b2, ESMK_DT_F32, E);
        if (!strcmp(sub, "self_attn_layer_norm.weight")) return put(o.ln1g, ESMK_DT_F32, E);
        if (!strcmp(sub, "self_attn_layer_norm.bias")) return put(o.ln1b, ESMK_DT_F32, E);
        if (!strcmp(sub, "final_layer_norm.weight")) return put(o.ln2g, ESMK_DT_F32, E);
        if (!strcmp(sub, "final_layer_norm.bias")) return put(o.ln2b, ESMK_DT_F32, E);
        return 0;  // e.g. self_attn.rot_emb.inv_freq: rebuilt in fp32 by the engine
    }
    return 0;  // unknown keys are ignored
}

int esmk_set_stream_edits(esmk_model* m, const esmk_stream_edit* edits, int n) {
    if (!m) return fail("esmk_set_stream_edits: null model");
    if (m->is_msa)
        return fail("esmk_set_stream_edits: MSA handle (stream edits are built for the ESM-2 / ESM-1b / ESM-1 stack; the esmk_msa_* "
                    "entries run without them)");
    if (n < 0 || n > ESMK_MAX_STREAM_EDITS)
        return fail("esmk_set_stream_edits: n must be 0 (clear) .. " + std::to_string(ESMK_MAX_STREAM_EDITS));
    if (n > 0 && !edits) return fail("esmk_set_stream_edits: null edit list");
    for (int i = 0; i < n; ++i)
        if (check_stream_edit("esmk_set_stream_edits: edit " + std::to_string(i), edits[i], m->E, m->L)) return 1;
    m->edits.assign(edits, edits + n);  // (a refused list leaves the edits that were set)
    return 0;
}

int esmk_set_layer_limit(esmk_model* m, int n_layers) {
    if (!m) return fail("esmk_set_layer_limit: null model");
    if (m->is_msa)
        return fail("esmk_set_layer_limit: MSA handle (the early exit is built for the ESM-2 / ESM-1b / ESM-1 stack; the esmk_msa_* "
                    "entries run the whole stack)");
    if (n_layers < 0 || n_layers > m->L)
        return fail("esmk_set_layer_limit: n_layers must be 0 (the whole stack) .. " + std::to_string(m->L));
    m->layer_limit = n_layers == m->L ? 0 : n_layers;
    return 0;
}

int esmk_workspace_bytes(const esmk_model* m, int B, int T, uint32_t out_flags, size_t* bytes) {
    if (!m || !bytes) return fail("esmk_workspace_bytes: null argument");
    if (m->is_msa) return fail("esmk_workspace_bytes: MSA handle (use esmk_msa_workspace_bytes)");
    if (B <= 0 || T <= 0) return fail("esmk_workspace_bytes: B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail("esmk_workspace_bytes: B*T exceeds 2^24 rows");
    *bytes = plan_workspace(m, B, T, out_flags).total;
    return 0;
}

int esmk_forward(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                 const int32_t* repr_layers, int n_repr, void* const* repr_out_dev,
                 uint32_t out_flags, void* logits_out_dev, void* attn_out_dev,
                 void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes,
                 void* stream) {
    ForwardCall c;
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.T = T;
    c.repr_layers = repr_layers, c.n_repr = n_repr, c.repr_out = repr_out_dev;
    c.flags = out_flags, c.logits = logits_out_dev, c.attn = attn_out_dev, c.contacts = contacts_out_dev;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return forward_impl(c);
}

// ---- variant scoring: log-probabilities of selected rows (examples/variant-prediction/predict.py) ---------
static int check_rows(const char* who, const esmk_model* m, int B, int T, int n_sel) {
    const std::string w(who);
    if (m->is_msa) return fail(w + ": MSA handle (the MSA Transformer has no row-selected forward)");
    if (B <= 0 || T <= 0) return fail(w + ": B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    if (n_sel <= 0) return fail(w + ": n_sel must be positive");
    if (n_sel > ESMK_MAX_ROWS) return fail(w + ": n_sel exceeds 2^24 rows");
    if (m->V > 64) return fail(w + ": vocabulary above 64 entries (the log-softmax holds one entry per lane)");
    return 0;
}

int esmk_rows_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset) {
    if (!m || !bytes) return fail("esmk_rows_workspace_bytes: null argument");
    if (check_rows("esmk_rows_workspace_bytes", m, B, T, n_sel)) return 1;
    RowSel rs;
    *bytes = plan_rows(m, B, T, n_sel, &rs);
    if (logits_offset) *logits_offset = rs.logits;
    return 0;
}

int esmk_forward_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                      const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream) {
    if (!m || !packed_dev || !tokens_dev || !sel_rows_dev || !logprobs_out_dev || !workspace_dev)
        return fail("esmk_forward_rows: null argument");
    if (check_rows("esmk_forward_rows", m, B, T, n_sel)) return 1;
    RowSel rs;
    if (workspace_bytes < plan_rows(m, B, T, n_sel, &rs)) return fail("esmk_forward_rows: workspace too small");
    if (!m->cfg.no_rope && m->inv_freq.empty()) return fail("esmk_forward_rows: esmk_set_rope_inv_freq was not called");
    rs.sel_dev = sel_rows_dev;
    rs.n_sel = n_sel;
    rs.logprobs_out = logprobs_out_dev;
    ForwardCall c;
    c.who = "esmk_forward_rows";
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.T = T;
    c.flags = ESMK_OUT_LOGITS, c.logits = (char*)workspace_dev + rs.logits;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.rs = &rs;
    return forward_impl(c);
}

// ---- design toward a target contact map: selected log-prob rows and pinned contact maps in one forward ----
// The head-group count of B = 1, whatever B is (include/esmk.h: the pin); 0 = the batch's own under the measurement switch
static int pinned_contact_groups(const esmk_model* m, int T) {
    if (esmk_host::g_rows_contacts_own_groups) return 0;
    const long long nQ = (T + 127) / 128;
    return contacts_head_groups(nQ * nQ, m->H, head_slots(m));
}

static int check_rows_contacts(const char* who, const esmk_model* m, int B, int T, int n_sel) {
    const std::string w(who);
    if (m->is_msa) return fail(w + ": MSA handle (the MSA Transformer has no row-selected forward with contact maps)");
    if (B <= 0 || T <= 0) return fail(w + ": B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    if (n_sel < 0) return fail(w + ": n_sel must not be negative");
    if (n_sel > ESMK_MAX_ROWS) return fail(w + ": n_sel exceeds 2^24 rows");
    if (n_sel > 0 && m->V > 64) return fail(w + ": vocabulary above 64 entries (the log-softmax holds one entry per lane)");
    if (T - (m->cfg.prepend_bos ? 1 : 0) - (m->cfg.append_eos ? 1 : 0) <= 0)
        return fail(w + ": no residue between <cls> and <eos>: the contact map is empty");
    return 0;
}

int esmk_rows_contacts_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset) {
    if (!m || !bytes) return fail("esmk_rows_contacts_workspace_bytes: null argument");
    if (check_rows_contacts("esmk_rows_contacts_workspace_bytes", m, B, T, n_sel)) return 1;
    RowSel rs;
    *bytes = plan_rows(m, B, T, n_sel, &rs, 0, ESMK_OUT_CONTACTS, pinned_contact_groups(m, T));
    if (logits_offset) *logits_offset = rs.logits;
    return 0;
}

int esmk_forward_rows_contacts(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                               const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, float* contacts_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!m || !packed_dev || !tokens_dev || !contacts_out_dev || !workspace_dev || (n_sel > 0 && (!sel_rows_dev || !logprobs_out_dev)))
        return fail("esmk_forward_rows_contacts: null argument");
    if (check_rows_contacts("esmk_forward_rows_contacts", m, B, T, n_sel)) return 1;
    RowSel rs;
    const int G = pinned_contact_groups(m, T);
    if (workspace_bytes < plan_rows(m, B, T, n_sel, &rs, 0, ESMK_OUT_CONTACTS, G))
        return fail("esmk_forward_rows_contacts: workspace too small");
    if (!m->cfg.no_rope && m->inv_freq.empty()) return fail("esmk_forward_rows_contacts: esmk_set_rope_inv_freq was not called");
    rs.sel_dev = sel_rows_dev;
    rs.n_sel = n_sel;
    rs.logprobs_out = logprobs_out_dev;
    ForwardCall c;
    c.who = "esmk_forward_rows_contacts";
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.T = T;
    c.flags = ESMK_OUT_CONTACTS | (n_sel > 0 ? ESMK_OUT_LOGITS : 0);
    c.logits = n_sel > 0 ? (char*)workspace_dev + rs.logits : nullptr;
    c.contacts = contacts_out_dev;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.rs = &rs;
    c.ct_G = G;
    return forward_impl(c);
}

// ---- linear pairwise heads on the attention maps (pair_head.hip) -------------------------------------------------
int esmk_set_pair_head(esmk_model* m, const float* w_host, const float* bias_host, int n_sym, int n_asym) {
    if (!m) return fail("esmk_set_pair_head: null model");
    if (m->is_msa)
        return fail("esmk_set_pair_head: MSA handle (the pairwise head is built for the ESM-2 / ESM-1b / ESM-1 stack; the MSA "
                    "Transformer's row attention maps have no such path)");
    if (n_sym < 0 || n_asym < 0) return fail("esmk_set_pair_head: n_sym and n_asym must not be negative");
    if (n_sym + n_asym > 64) return fail("esmk_set_pair_head: n_sym + n_asym must be 0 (clear) .. 64");
    const int C_out = n_sym + n_asym;
    if (C_out > 0 && (!w_host || !bias_host)) return fail("esmk_set_pair_head: null weight or bias");
    if (C_out == 0) {
        m->pair_sym = m->pair_asym = 0;  // (the device copies stay for the next head)
        return 0;
    }
    const size_t C = (size_t)m->L * m->H;
    std::vector<float> w64(C * 64, 0.f);
    for (size_t c = 0; c < C; ++c) memcpy(&w64[c * 64], w_host + c * C_out, (size_t)C_out * 4);
    // (a forward in flight on another stream may still read the old copies)
    ESMK_TRY(hipDeviceSynchronize());
    if (!m->d_pair_w64) ESMK_TRY(hipMalloc(&m->d_pair_w64, C * 64 * 4));
    if (!m->d_pair_bias) ESMK_TRY(hipMalloc(&m->d_pair_bias, 64 * 4));
    ESMK_TRY(hipMemcpy(m->d_pair_w64, w64.data(), C * 64 * 4, hipMemcpyHostToDevice));
    ESMK_TRY(hipMemcpy(m->d_pair_bias, bias_host, (size_t)C_out * 4, hipMemcpyHostToDevice));
    m->pair_sym = n_sym;
    m->pair_asym = n_asym;
    return 0;
}

static int check_rows_pair(const char* who, const esmk_model* m, int B, int T, int n_sel) {
    const std::string w(who);
    if (m->is_msa) return fail(w + ": MSA handle (the MSA Transformer has no pairwise head on its attention maps)");
    if (m->pair_sym + m->pair_asym <= 0) return fail(w + ": no pairwise head is set (esmk_set_pair_head)");
    if (B <= 0 || T <= 0) return fail(w + ": B and T must be positive");
    if ((long long)B * T > ESMK_MAX_ROWS) return fail(w + ": B*T exceeds 2^24 rows");
    if (n_sel < 0) return fail(w + ": n_sel must not be negative");
    if (n_sel > ESMK_MAX_ROWS) return fail(w + ": n_sel exceeds 2^24 rows");
    if (n_sel > 0 && m->V > 64) return fail(w + ": vocabulary above 64 entries (the log-softmax holds one entry per lane)");
    if (T - (m->cfg.prepend_bos ? 1 : 0) - (m->cfg.append_eos ? 1 : 0) <= 0)
        return fail(w + ": no residue between <cls> and <eos>: the pair map is empty");
    return 0;
}

int esmk_rows_pair_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset) {
    if (!m || !bytes) return fail("esmk_rows_pair_workspace_bytes: null argument");
    if (check_rows_pair("esmk_rows_pair_workspace_bytes", m, B, T, n_sel)) return 1;
    RowSel rs;
    PairStash ps;
    *bytes = plan_rows_pair(m, B, T, n_sel, &rs, &ps);
    if (logits_offset) *logits_offset = rs.logits;
    return 0;
}

int esmk_forward_rows_pair(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                           const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, float* pair_out_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!m || !packed_dev || !tokens_dev || !pair_out_dev || !workspace_dev || (n_sel > 0 && (!sel_rows_dev || !logprobs_out_dev)))
        return fail("esmk_forward_rows_pair: null argument");
    if (check_rows_pair("esmk_forward_rows_pair", m, B, T, n_sel)) return 1;
    RowSel rs;
    PairStash ps;
    if (workspace_bytes < plan_rows_pair(m, B, T, n_sel, &rs, &ps)) return fail("esmk_forward_rows_pair: workspace too small");
    if (!m->cfg.no_rope && m->inv_freq.empty()) return fail("esmk_forward_rows_pair: esmk_set_rope_inv_freq was not called");
    rs.sel_dev = sel_rows_dev;
    rs.n_sel = n_sel;
    rs.logprobs_out = logprobs_out_dev;
    ps.out = pair_out_dev;
    ForwardCall c;
    c.who = "esmk_forward_rows_pair";
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.T = T;
    c.flags = n_sel > 0 ? ESMK_OUT_LOGITS : 0;
    c.logits = n_sel > 0 ? (char*)workspace_dev + rs.logits : nullptr;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.rs = &rs;
    c.ps = &ps;
    return forward_impl(c);
}

int esmk_debug_contact_groups(const esmk_model* m, int B, int T, int pinned, int32_t* groups) {
    if (!m || !groups) return fail("esmk_debug_contact_groups: null argument");
    if (m->is_msa) return fail("esmk_debug_contact_groups: MSA handle (its contact head reads the row attention maps)");
    if (B <= 0 || T <= 0) return fail("esmk_debug_contact_groups: B and T must be positive");
    const long long nQ = (T + 127) / 128;
    *groups = contacts_head_groups((pinned ? 1 : (long long)B) * nQ * nQ, m->H, head_slots(m));
    return 0;
}

// ---- token-packed batches (no compute on padding) --------------------------------------
static int check_segments(const char* who, const esmk_model* m, const int32_t* seg, int n_seg, int rows,
                          PackedCtx* pc) {
    const std::string w(who);
    if (!m || !seg) return fail(w + ": null argument");
    if (m->is_msa) return fail(w + ": not an ESM-2 handle");
    if (m->esm1) return fail(w + ": ESM-1 (no_rope = ESMK_ESM1) runs padded batches only (esmk_forward); it has no token-packed form yet");
    SegTableInfo info;
    if (check_seg_table(w, seg, n_seg, rows, false, &info)) return 1;
    pc->n_seg = n_seg;
    pc->max_len = info.max_len;
    pc->n_items = (int)info.items;
    pc->sum_len2 = info.sum_len2;
    pc->seg_host = seg;
    return 0;
}

int esmk_packed_workspace_bytes(const esmk_model* m, int n_seg, int rows, uint32_t out_flags, size_t* bytes) {
    if (!m || !bytes) return fail("esmk_packed_workspace_bytes: null argument");
    if (m->is_msa) return fail("esmk_packed_workspace_bytes: not an ESM-2 handle");
    if (m->esm1)
        return fail("esmk_packed_workspace_bytes: ESM-1 (no_rope = ESMK_ESM1) runs padded batches only (esmk_forward); it has no token-packed form yet");
    if (n_seg <= 0 || rows <= 0 || rows % 64 != 0 || rows > ESMK_MAX_ROWS)
        return fail("esmk_packed_workspace_bytes: need n_seg > 0 and 0 < rows <= 2^24, rows % 64 == 0");
    if (out_flags & ~(uint32_t)(ESMK_OUT_LOGITS | ESMK_OUT_REPR_LOWP))
        return fail("esmk_packed_workspace_bytes: only ESMK_OUT_LOGITS / ESMK_OUT_REPR_LOWP are available");
    *bytes = plan_workspace(m, 1, rows, out_flags, n_seg).total;
    return 0;
}

// The _ex and _maps entries (workspace query and forward): handle, segment table and flag checks; `allowed`: the flags of the
// entry, `only`: their names.  With ESMK_OUT_CONTACTS the contact plan of the batch is made in *ct.  The map flags never
// reach forward_impl (contacts stay the fused per-segment form): they travel in the PackedCtx.
constexpr uint32_t kMapFlags = ESMK_OUT_ATTN | ESMK_OUT_ATTN_LOWP;
constexpr uint32_t kPackedExFlags = ESMK_OUT_LOGITS | ESMK_OUT_REPR_LOWP | ESMK_OUT_CONTACTS;
static const char* const kPackedExOnly = "ESMK_OUT_LOGITS / ESMK_OUT_REPR_LOWP / ESMK_OUT_CONTACTS";
static const char* const kPackedMapsOnly = "ESMK_OUT_LOGITS / ESMK_OUT_REPR_LOWP / ESMK_OUT_CONTACTS / ESMK_OUT_ATTN / ESMK_OUT_ATTN_LOWP";
static int check_packed(const char* who, const esmk_model* m, const int32_t* seg, int n_seg, int rows, uint32_t out_flags,
                        uint32_t allowed, const char* only, PackedCtx* pc, CtPackedPlan* ct) {
    const std::string w(who);
    if (check_segments(who, m, seg, n_seg, rows, pc)) return 1;
    if ((out_flags & kMapFlags & ~allowed) != 0) return fail(w + ": attention maps take padded batches (esmk_forward)");
    if (out_flags & ~allowed) return fail(w + ": only " + only + " are available");
    if (split_x3(m))
        return fail(w + ": the f16x3 precision mode runs padded batches of head_dim-64 models (no token-packed form)");
    if (out_flags & ESMK_OUT_CONTACTS) {
        *ct = contacts_packed_plan(seg, n_seg, m->H, head_slots(m), m->cfg.prepend_bos ? 1 : 0, m->cfg.append_eos ? 1 : 0);
        pc->ct = ct;
    }
    pc->maps = (out_flags & kMapFlags) != 0;
    pc->maps_lowp = (out_flags & ESMK_OUT_ATTN_LOWP) != 0;
    return 0;
}

int esmk_packed_workspace_bytes_ex(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows,
                                   uint32_t out_flags, size_t* bytes) {
    if (!m || !bytes) return fail("esmk_packed_workspace_bytes_ex: null argument");
    PackedCtx pc;
    CtPackedPlan ct;
    if (check_packed("esmk_packed_workspace_bytes_ex", m, segments_host, n_seg, rows, out_flags, kPackedExFlags, kPackedExOnly, &pc, &ct))
        return 1;
    *bytes = plan_workspace(m, 1, rows, out_flags, n_seg, pc.ct).total;
    return 0;
}

// a token-packed forward: B = 1, T = rows
static ForwardCall packed_call(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int rows,
                               const int32_t* repr_layers, int n_repr, void* const* repr_out_dev, uint32_t out_flags,
                               void* logits_out_dev, void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream, const PackedCtx* pc) {
    ForwardCall c;
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = 1, c.T = rows;
    c.repr_layers = repr_layers, c.n_repr = n_repr, c.repr_out = repr_out_dev;
    c.flags = out_flags, c.logits = logits_out_dev, c.contacts = contacts_out_dev;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.pc = pc;
    return c;
}

int esmk_forward_packed_ex(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                           const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers,
                           int n_repr, void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev,
                           void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    PackedCtx pc;
    CtPackedPlan ct;
    if (check_packed("esmk_forward_packed_ex", m, segments_host, n_seg, rows, out_flags, kPackedExFlags, kPackedExOnly, &pc, &ct))
        return 1;
    return forward_impl(packed_call(m, packed_dev, tokens_dev, rows, repr_layers, n_repr, repr_out_dev, out_flags,
                                    logits_out_dev, contacts_out_dev, workspace_dev, workspace_bytes, stream, &pc));
}

int esmk_packed_workspace_bytes_maps(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows,
                                     uint32_t out_flags, size_t* bytes) {
    if (!m || !bytes) return fail("esmk_packed_workspace_bytes_maps: null argument");
    PackedCtx pc;
    CtPackedPlan ct;
    if (check_packed("esmk_packed_workspace_bytes_maps", m, segments_host, n_seg, rows, out_flags, kPackedExFlags | kMapFlags,
                     kPackedMapsOnly, &pc, &ct))
        return 1;
    *bytes = plan_workspace(m, 1, rows, out_flags & ~kMapFlags, n_seg, pc.ct, pc.maps).total;
    return 0;
}

int esmk_forward_packed_maps(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                             const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers, int n_repr,
                             void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev, void* attn_out_dev,
                             size_t attn_out_elems, void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream) {
    PackedCtx pc;
    CtPackedPlan ct;
    if (check_packed("esmk_forward_packed_maps", m, segments_host, n_seg, rows, out_flags, kPackedExFlags | kMapFlags,
                     kPackedMapsOnly, &pc, &ct))
        return 1;
    if (m->layer_limit > 0)
        return fail("esmk_forward_packed_maps: a layer limit of " + std::to_string(m->layer_limit) +
                    " is set (esmk_set_layer_limit): this entry needs the whole stack");
    if (pc.maps) {
        if (!attn_out_dev) return fail("esmk_forward_packed_maps: attention buffer missing");
        // sum(len^2) <= rows^2 <= 2^48 (check_seg_table): the product with L H stays inside 64 bits
        const unsigned long long need = pc.sum_len2 * (unsigned long long)m->L * (unsigned long long)m->H;
        if ((unsigned long long)attn_out_elems < need)
            return fail("esmk_forward_packed_maps: attention buffer too small (" + std::to_string(attn_out_elems) + " elements, need " +
                        std::to_string(need) + " = L H sum(len^2))");
        pc.maps_out = attn_out_dev;
    }
    return forward_impl(packed_call(m, packed_dev, tokens_dev, rows, repr_layers, n_repr, repr_out_dev, out_flags & ~kMapFlags,
                                    logits_out_dev, contacts_out_dev, workspace_dev, workspace_bytes, stream, &pc));
}

int esmk_forward_packed(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                        const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers,
                        int n_repr, void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream) {
    PackedCtx pc;
    if (check_segments("esmk_forward_packed", m, segments_host, n_seg, rows, &pc)) return 1;
    if (out_flags & ~(uint32_t)(ESMK_OUT_LOGITS | ESMK_OUT_REPR_LOWP))
        return fail("esmk_forward_packed: attention maps and contacts take padded batches (esmk_forward)");
    return forward_impl(packed_call(m, packed_dev, tokens_dev, rows, repr_layers, n_repr, repr_out_dev, out_flags,
                                    logits_out_dev, nullptr, workspace_dev, workspace_bytes, stream, &pc));
}

// ---- token-packed batch + row selection: mixed-length libraries of masked copies (predict.py:138-143,205-215) -------------
static int check_packed_rows(const char* who, const esmk_model* m, const int32_t* seg, int n_seg, int rows, int n_sel,
                             PackedCtx* pc) {
    if (check_segments(who, m, seg, n_seg, rows, pc)) return 1;
    if (split_x3(m))
        return fail(std::string(who) + ": the f16x3 precision mode runs padded batches of head_dim-64 models (no token-packed form)");
    return check_rows(who, m, 1, rows, n_sel);
}

int esmk_packed_rows_workspace_bytes(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows, int n_sel,
                                     size_t* bytes, size_t* logits_offset) {
    if (!m || !bytes) return fail("esmk_packed_rows_workspace_bytes: null argument");
    PackedCtx pc;
    if (check_packed_rows("esmk_packed_rows_workspace_bytes", m, segments_host, n_seg, rows, n_sel, &pc)) return 1;
    RowSel rs;
    *bytes = plan_rows(m, 1, rows, n_sel, &rs, n_seg);
    if (logits_offset) *logits_offset = rs.logits;
    return 0;
}

int esmk_forward_packed_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, const int32_t* segments_host,
                             int n_seg, int rows, const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!m || !packed_dev || !tokens_dev || !segments_host || !sel_rows_dev || !logprobs_out_dev || !workspace_dev)
        return fail("esmk_forward_packed_rows: null argument");
    PackedCtx pc;
    if (check_packed_rows("esmk_forward_packed_rows", m, segments_host, n_seg, rows, n_sel, &pc)) return 1;
    if (refuse_edits_packed("esmk_forward_packed_rows", m)) return 1;
    RowSel rs;
    if (workspace_bytes < plan_rows(m, 1, rows, n_sel, &rs, n_seg)) return fail("esmk_forward_packed_rows: workspace too small");
    if (!m->cfg.no_rope && m->inv_freq.empty()) return fail("esmk_forward_packed_rows: esmk_set_rope_inv_freq was not called");
    rs.sel_dev = sel_rows_dev;
    rs.n_sel = n_sel;
    rs.logprobs_out = logprobs_out_dev;
    ForwardCall c;
    c.who = "esmk_forward_packed_rows";
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = 1, c.T = rows;
    c.flags = ESMK_OUT_LOGITS, c.logits = (char*)workspace_dev + rs.logits;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.pc = &pc;
    c.rs = &rs;
    return forward_impl(c);
}

int esmk_ln_fold_enabled(const esmk_model* m) { return (!m || m->is_msa) ? -1 : (m->fold ? 1 : 0); }

int esmk_profile_begin(esmk_model* m) {
    if (!m) return fail("esmk_profile_begin: null model");
    for (auto& r : m->prof) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    m->prof.clear();
    m->prof_on = true;
    return 0;
}

int esmk_profile_end(esmk_model* m, esmk_profile_entry* out, int max_entries, int* n_out) {
    if (!m || !out || !n_out) return fail("esmk_profile_end: null argument");
    m->prof_on = false;
    std::vector<esmk_profile_entry> agg(PC_COUNT);
    for (int c = 0; c < PC_COUNT; ++c) {
        memset(&agg[c], 0, sizeof(esmk_profile_entry));
        strncpy(agg[c].name, kProfNames[c], sizeof(agg[c].name) - 1);
    }
    for (auto& r : m->prof) {
        ESMK_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        ESMK_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        agg[r.cls].launches += 1;
        agg[r.cls].ms += ms;
        agg[r.cls].flops += r.flops;
        agg[r.cls].bytes += r.bytes;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    m->prof.clear();
    int n = 0;
    for (int c = 0; c < PC_COUNT && n < max_entries; ++c)
        if (agg[c].launches > 0) out[n++] = agg[c];
    *n_out = n;
    return 0;
}

}  // extern "C"
