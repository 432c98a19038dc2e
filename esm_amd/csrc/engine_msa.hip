// engine_msa.hip — host side of the MSA Transformer path of libesmk.so (declared in include/esmk.h):
// packed parameter layout, workspace planning and the launch sequence that replaces MSATransformer.forward
// (reference esm/model/msa_transformer.py:146-220).  Kernels live in gemm8.hip, attention.hip, elementwise.hip.
#include "engine_internal.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

using namespace esmk;
using namespace esmk_host;

namespace esmk_host {
void plan_packed_msa(esmk_model* m) {
    const size_t os = op_size(m->cfg.operand_dtype);
    const size_t E = m->E, F = m->F, V = m->V;
    // f16x2: every layer matrix as [rows, 2 cols] (hi | lo K tiles); f16x2a: the attention projections only
    const size_t ws = m->cfg.weight_split ? 2 : 1;
    const SplitPlan sp = split_plan(m);
    Carve c;
    m->embed_f32 = c.take(V * E * 4);
    m->embed_op = c.take(V * E * os);
    m->pos_emb = c.take((size_t)m->npos * E * 4);
    m->msa_pos = c.take((size_t)1024 * E * 4);
    m->lnb_g = c.take(E * 4);
    m->lnb_b = c.take(E * 4);
    m->fin_g = c.take(E * 4);
    m->fin_b = c.take(E * 4);
    m->lm_w = c.take(E * E * os);
    m->lm_w32 = c.take(ws == 2 ? E * E * 4 : 0);
    m->lm_b = c.take(E * 4);
    m->lm_lng = c.take(E * 4);
    m->lm_lnb = c.take(E * 4);
    m->lm_bias = c.take(V * 4);
    m->ct_w = c.take((size_t)m->L * m->H * 4);
    m->ct_b = c.take(4);
    m->mlayer.resize(m->L);
    auto attn = [&](AttnOff& a) {
        a.wqkv = c.take(E * E * os * (2 * sp.qk + sp.v));
        a.bqkv = c.take(3 * E * 4);
        a.wo = c.take(E * E * os * sp.o);
        a.bo = c.take(E * 4);
        a.lng = c.take(E * 4);
        a.lnb = c.take(E * 4);
    };
    for (int l = 0; l < m->L; ++l) {
        MsaLayerOff& o = m->mlayer[l];
        attn(o.row);
        attn(o.col);
        o.w1 = c.take(F * E * os * sp.ffn);
        o.b1 = c.take(F * 4);
        o.w2 = c.take(E * F * os * sp.ffn);
        o.b2 = c.take(E * 4);
        o.flng = c.take(E * 4);
        o.flnb = c.take(E * 4);
    }
    m->packed_bytes = c.off;
}
}  // namespace esmk_host

// =============================================================================================
// MSA Transformer (reference esm/model/msa_transformer.py, esm/axial_attention.py)
// =============================================================================================
namespace {

struct MsaWorkspace {
    size_t keep, col_fill, any_pad, x, h, big, scores, probs, lse, ct_scratch, total;
    size_t q, k, vt;  // inside big
    int Cp, Rp;
    int row_slices;  // the tied-score GEMM sums over R rows in this many K slices (partial maps summed by the softmax)
};

// Tied row attention scores: per (b, head) a [C, C] map contracted over R * 64, i.e. only B * H * ceil(C/256)^2
// output tiles (108 for one 128 x 513 MSA) with a very long K loop: less than half of the 256 CUs would work.
// The contraction is cut into `S` slices of R / S rows (S | R), each slice a batch entry of the same persistent
// GEMM writing its own fp32 partial map; msa_row_softmax_kernel adds the slices in index order (deterministic).
int row_score_slices(int B, int H, int R, int C) {
    const int tiles = B * H * ((C + 255) / 256) * ((C + 255) / 256);
    int best = 1;
    for (int s = 2; s <= 8 && s * tiles <= 256 + tiles / 2; ++s)
        if (R % s == 0) best = s;
    return best;
}

// slices_B: the batch size the slice count of the tied-score GEMM is chosen for — B itself (esmk_msa_forward), or 1
// (esmk_msa_forward_rows: every copy of the batch then runs the launches and summation order of a B = 1 forward)
MsaWorkspace plan_msa_workspace(const esmk_model* m, int B, int R, int C, uint32_t flags, int slices_B) {
    MsaWorkspace w{};
    const size_t os = op_size(m->cfg.operand_dtype);
    const size_t N = (size_t)B * R * C, E = m->E, F = m->F, H = m->H;
    w.Cp = (C + 63) / 64 * 64;
    w.Rp = (R + 63) / 64 * 64;
    Carve c;
    w.keep = c.take(N * 4);
    w.col_fill = c.take(N * 4);
    w.any_pad = c.take(256);
    w.x = c.take(N * E * 4);
    w.h = c.take(N * E * os + 4096);
    const size_t qb = align_up(N * E * os + 4096);
    const size_t vt_row = (size_t)B * H * R * 64 * w.Cp * os;         // [B,H,R,64,Cp]
    const size_t vt_col = (size_t)B * C * H * 64 * w.Rp * os;         // [B*C,H,64,Rp]
    size_t big = 2 * qb + align_up(std::max(vt_row, vt_col));
    big = std::max(big, N * F * os);
    big = std::max(big, N * E * 4);
    w.big = c.take(big);
    w.q = w.big;
    w.k = w.big + qb;
    w.vt = w.big + 2 * qb;
    w.row_slices = row_score_slices(slices_B, (int)H, R, C);
    w.scores = c.take((size_t)w.row_slices * B * H * C * w.Cp * 4);
    w.probs = c.take((size_t)B * H * C * w.Cp * os);
    w.lse = c.take((flags & ESMK_OUT_COL_ATTN) ? (size_t)B * C * H * R * 4 : 0);
    const int S = C - (m->cfg.prepend_bos ? 1 : 0) - (m->cfg.append_eos ? 1 : 0);
    w.ct_scratch =
        c.take((flags & ESMK_OUT_CONTACTS) ? (size_t)B * m->L * m->H * (size_t)(S > 0 ? S + 1 : 1) * 4 : 0);
    w.total = c.off;
    return w;
}

// Row selection (esmk_msa_forward_rows): the layer stack runs on all B*R*C rows, the head of the model — final LayerNorm, LM
// head, vocabulary GEMM — on the n_sel gathered rows only, and a log-softmax turns their logits into logprobs_out.
struct MsaRowSel {
    const int32_t* sel_dev = nullptr;  // int32 [n_sel] flat indices (b*R + r)*C + c, device data: clamped by the gather kernel
    int n_sel = 0;
    float* logprobs_out = nullptr;     // fp32 [n_sel, V]
    size_t x = 0, h = 0, g32 = 0, logits = 0;  // byte offsets into the workspace
};

// esmk_msa_forward_rows: the forward's workspace with the slice count of B = 1 (it is never below the count of B: the scores
// buffer only grows), then the selected rows of the stream (fp32), their operand-dtype rows, the fp32 scratch of the head
// and the selected logits.  No pad rows: every GEMM kernel clamps its A-row reads to row M - 1.
size_t plan_msa_rows(const esmk_model* m, int B, int R, int C, int n_sel, MsaRowSel* rs) {
    Carve c;
    c.take(plan_msa_workspace(m, B, R, C, ESMK_OUT_LOGITS, 1).total);
    const size_t n = (size_t)n_sel;
    rs->x = c.take(n * m->E * 4);
    rs->h = c.take(n * m->E * op_size(m->cfg.operand_dtype) + 4096);
    rs->g32 = c.take(n * m->E * 4);
    rs->logits = c.take(n * m->V * 4);
    return c.off;
}

// One call of the MSA forward: the arguments of esmk_msa_forward, or (rs) of esmk_msa_forward_rows
struct MsaCall {
    const char* who = "esmk_msa_forward";  // the entry error messages name
    esmk_model* m = nullptr;
    const void* packed = nullptr;
    const int64_t* tokens = nullptr;
    int B = 0, R = 0, C = 0;
    const int32_t* repr_layers = nullptr;
    int n_repr = 0;
    void* const* repr_out = nullptr;
    uint32_t flags = 0;
    void *logits = nullptr, *row_attn = nullptr, *col_attn = nullptr, *contacts = nullptr;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    void* stream = nullptr;
    const MsaRowSel* rs = nullptr;
};

// the shape limits of both entries (and of the rows entry's workspace query)
int check_msa_shape(const std::string& w, const esmk_model* m, int B, int R, int C) {
    if (B <= 0 || R <= 0 || C <= 0) return fail(w + ": B, R, C must be positive");
    if ((long long)B * R * C > ESMK_MAX_ROWS) return fail(w + ": B*R*C exceeds 2^24 rows");
    if (R > 1024 && m->has_msa_pos)
        return fail(w + ": MSA position embedding covers a depth of 1024 alignments");  // msa_transformer.py:160-164
    if (C > 1024) return fail(w + ": more than 1024 columns are not supported");
    if (C > m->npos - m->cfg.pad_idx - 1)
        return fail(w + ": sequence length above the maximum of the positional embedding");  // modules.py:243-247
    return 0;
}

int check_msa_rows(const char* who, const esmk_model* m, int B, int R, int C, int n_sel) {
    const std::string w(who);
    if (!m->is_msa) return fail(w + ": not an MSA model handle (esmk_forward_rows takes the single-sequence models)");
    if (check_msa_shape(w, m, B, R, C)) return 1;
    if (n_sel <= 0) return fail(w + ": n_sel must be positive");
    if (n_sel > ESMK_MAX_ROWS) return fail(w + ": n_sel exceeds 2^24 rows");
    if (m->V > 64) return fail(w + ": vocabulary above 64 entries (the log-softmax holds one entry per lane)");
    return 0;
}

int msa_forward_impl(const MsaCall& c);

}  // namespace

extern "C" {

int esmk_msa_create(const esmk_msa_config* cfg, esmk_model** out) {
    if (!cfg || !out) return fail("esmk_msa_create: null argument");
    if (cfg->num_layers <= 0 || cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->ffn_dim <= 0 ||
        cfg->vocab <= 0 || cfg->num_positions <= 0)
        return fail("esmk_msa_create: non-positive dimension");
    if (cfg->embed_dim % cfg->num_heads != 0 || cfg->embed_dim / cfg->num_heads != 64)
        return fail("esmk_msa_create: head_dim must be 64 for the gfx950 attention kernels");
    if (cfg->embed_dim % 64 != 0 || cfg->ffn_dim % 64 != 0)
        return fail("esmk_msa_create: embed_dim and ffn_dim must be multiples of 64");
    if (cfg->operand_dtype != ESMK_F16 && cfg->operand_dtype != ESMK_BF16)
        return fail("esmk_msa_create: operand_dtype must be ESMK_F16 or ESMK_BF16");
    if (cfg->weight_split < 0 || cfg->weight_split > 3) return fail("esmk_msa_create: weight_split must be 0 (off), 1 (f16x2), 2 (f16x2a) or 3 (f16x2v)");
    if (cfg->weight_split != 0 && cfg->operand_dtype != ESMK_F16)
        return fail("esmk_msa_create: weight_split (precision modes f16x2 / f16x2a / f16x2v) needs operand_dtype ESMK_F16");
    esmk_model* m = new esmk_model();
    memset(&m->cfg, 0, sizeof(m->cfg));
    m->cfg.num_layers = cfg->num_layers;
    m->cfg.embed_dim = cfg->embed_dim;
    m->cfg.num_heads = cfg->num_heads;
    m->cfg.ffn_dim = cfg->ffn_dim;
    m->cfg.vocab = cfg->vocab;
    m->cfg.pad_idx = cfg->pad_idx;
    m->cfg.mask_idx = cfg->mask_idx;
    m->cfg.cls_idx = cfg->cls_idx;
    m->cfg.eos_idx = cfg->eos_idx;
    m->cfg.prepend_bos = cfg->prepend_bos;
    m->cfg.append_eos = cfg->append_eos;
    m->cfg.operand_dtype = cfg->operand_dtype;
    m->cfg.weight_split = cfg->weight_split;
    m->L = cfg->num_layers;
    m->E = cfg->embed_dim;
    m->H = cfg->num_heads;
    m->F = cfg->ffn_dim;
    m->V = cfg->vocab;
    m->D = 64;
    m->EA = m->E;
    m->Kp = m->E;
    m->is_msa = true;
    m->npos = cfg->num_positions;
    m->has_msa_pos = cfg->has_msa_position_embedding;
    plan_packed_msa(m);
    *out = m;
    return 0;
}

int esmk_msa_workspace_bytes(const esmk_model* m, int B, int R, int C, uint32_t out_flags, size_t* bytes) {
    if (!m || !bytes || !m->is_msa) return fail("esmk_msa_workspace_bytes: not an MSA model handle");
    if (B <= 0 || R <= 0 || C <= 0) return fail("esmk_msa_workspace_bytes: B, R, C must be positive");
    if ((long long)B * R * C > ESMK_MAX_ROWS) return fail("esmk_msa_workspace_bytes: B*R*C exceeds 2^24 rows");
    *bytes = plan_msa_workspace(m, B, R, C, out_flags, B).total;
    return 0;
}

int esmk_msa_forward(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int R, int C,
                     const int32_t* repr_layers, int n_repr, void* const* repr_out_dev, uint32_t out_flags,
                     void* logits_out_dev, void* row_attn_out_dev, void* col_attn_out_dev,
                     void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    MsaCall c;
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.R = R, c.C = C;
    c.repr_layers = repr_layers, c.n_repr = n_repr, c.repr_out = repr_out_dev;
    c.flags = out_flags, c.logits = logits_out_dev, c.row_attn = row_attn_out_dev, c.col_attn = col_attn_out_dev;
    c.contacts = contacts_out_dev;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return msa_forward_impl(c);
}

// ---- variant scoring with the MSA Transformer: log-probabilities of selected rows (predict.py:161-184) ----
int esmk_msa_rows_workspace_bytes(const esmk_model* m, int B, int R, int C, int n_sel, size_t* bytes, size_t* logits_offset) {
    if (!m || !bytes) return fail("esmk_msa_rows_workspace_bytes: null argument");
    if (check_msa_rows("esmk_msa_rows_workspace_bytes", m, B, R, C, n_sel)) return 1;
    MsaRowSel rs;
    *bytes = plan_msa_rows(m, B, R, C, n_sel, &rs);
    if (logits_offset) *logits_offset = rs.logits;
    return 0;
}

int esmk_msa_forward_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int R, int C,
                          const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream) {
    if (!m || !packed_dev || !tokens_dev || !sel_rows_dev || !logprobs_out_dev || !workspace_dev)
        return fail("esmk_msa_forward_rows: null argument");
    if (check_msa_rows("esmk_msa_forward_rows", m, B, R, C, n_sel)) return 1;
    MsaRowSel rs;
    if (workspace_bytes < plan_msa_rows(m, B, R, C, n_sel, &rs)) return fail("esmk_msa_forward_rows: workspace too small");
    rs.sel_dev = sel_rows_dev;
    rs.n_sel = n_sel;
    rs.logprobs_out = logprobs_out_dev;
    MsaCall c;
    c.who = "esmk_msa_forward_rows";
    c.m = m, c.packed = packed_dev, c.tokens = tokens_dev, c.B = B, c.R = R, c.C = C;
    c.flags = ESMK_OUT_LOGITS, c.logits = (char*)workspace_dev + rs.logits;
    c.workspace = workspace_dev, c.workspace_bytes = workspace_bytes, c.stream = stream;
    c.rs = &rs;
    return msa_forward_impl(c);
}

int esmk_debug_msa_row_slices(const esmk_model* m, int B, int R, int C, int rows_entry, int32_t* slices) {
    if (!m || !slices || !m->is_msa) return fail("esmk_debug_msa_row_slices: not an MSA model handle");
    if (check_msa_shape("esmk_debug_msa_row_slices", m, B, R, C)) return 1;
    *slices = plan_msa_workspace(m, B, R, C, ESMK_OUT_LOGITS, rows_entry ? 1 : B).row_slices;
    return 0;
}

}  // extern "C"

namespace {

// The implementation of both entries: argument checks under the caller's name, then the launch sequence.  Whatever the
// entry, copy b of the batch goes through the same kernels; what the rows entry changes is the slice count of the tied-score
// GEMM (pinned to B = 1) and the rows the head of the model runs on.
int msa_forward_impl(const MsaCall& c) {
    esmk_model* m = c.m;
    const std::string who(c.who);
    const int B = c.B, R = c.R, C = c.C;
    const uint32_t out_flags = c.flags;
    const int32_t* repr_layers = c.repr_layers;
    const int n_repr = c.n_repr;
    void* const* repr_out_dev = c.repr_out;
    const int64_t* tokens_dev = c.tokens;
    void *row_attn_out_dev = c.row_attn, *col_attn_out_dev = c.col_attn, *contacts_out_dev = c.contacts;
    if (!m || !m->is_msa) return fail(who + ": not an MSA model handle");
    if (!c.packed || !tokens_dev || !c.workspace) return fail(who + ": null argument");
    if (check_msa_shape(who, m, B, R, C)) return 1;
    if (out_flags & (ESMK_OUT_REPR_LOWP | ESMK_OUT_ATTN_LOWP))
        return fail(who + ": outputs are fp32 (ESMK_OUT_*_LOWP is an esmk_forward flag)");
    const bool want_logits = out_flags & ESMK_OUT_LOGITS;
    const bool want_contacts = out_flags & ESMK_OUT_CONTACTS;
    const bool want_attn = (out_flags & ESMK_OUT_ATTN) || want_contacts;
    if (want_logits && !c.logits) return fail(who + ": logits buffer missing");
    if (want_attn && !row_attn_out_dev) return fail(who + ": row attention buffer missing");
    if (want_contacts && !contacts_out_dev) return fail(who + ": contacts buffer missing");
    const bool want_col = out_flags & ESMK_OUT_COL_ATTN;
    if (want_col && !col_attn_out_dev) return fail(who + ": column attention buffer missing");
    for (int i = 0; i < n_repr; ++i)
        if (repr_layers[i] < 0 || repr_layers[i] > m->L || !repr_out_dev[i])
            return fail(who + ": bad repr layer request");
    const MsaWorkspace w = plan_msa_workspace(m, B, R, C, out_flags, c.rs ? 1 : B);
    if (c.workspace_bytes < w.total) return fail(who + ": workspace too small");

    hipStream_t st = (hipStream_t)c.stream;
    const int op = m->cfg.operand_dtype;
    const size_t os = op_size(op);
    const int N = B * R * C, E = m->E, F = m->F, H = m->H, L = m->L, Cp = w.Cp, Rp = w.Rp;
    char* ws = (char*)c.workspace;
    const char* pk = (const char*)c.packed;
    float* keep = (float*)(ws + w.keep);
    float* col_fill = (float*)(ws + w.col_fill);
    int* any_pad = (int*)(ws + w.any_pad);
    float* x = (float*)(ws + w.x);
    void* h = ws + w.h;
    void* q = ws + w.q;
    void* k = ws + w.k;
    void* vt = ws + w.vt;
    void* ffn = ws + w.big;
    float* g32 = (float*)(ws + w.big);
    float* scores = (float*)(ws + w.scores);
    void* probs = ws + w.probs;
    if (ensure_unit_rope(m, std::max(R, C), st)) return 1;

    const double NE = (double)N * E;
    const Stack s{m, st, op, os, pk, N, repr_layers, n_repr, repr_out_dev};

    // msa_transformer.py:152-172: token + position + MSA-row embeddings, LayerNorm, pads zeroed
    {
        ProfScope ps(m, st, PC_EMBED, 0, (double)N * 8 + 4 * NE);
        ESMK_TRY(launch_msa_embed(tokens_dev, (const float*)(pk + m->embed_f32), (const float*)(pk + m->pos_emb),
                                  m->has_msa_pos ? (const float*)(pk + m->msa_pos) : nullptr, x, keep, col_fill,
                                  any_pad, B, R, C, E, m->V, m->cfg.pad_idx, m->npos, st));
    }
    {
        LnExtra ex;
        ex.row_keep = keep;
        if (s.lnorm(x, m->lnb_g, m->lnb_b, nullptr, x, N, ex)) return 1;
    }
    if (s.repr_copy(0, x)) return 1;

    // q/k/v projections of one axial attention block on `rows` = N rows grouped in sequences of T tokens
    auto qkv = [&](const AttnOff& a, int T, int Tp, float scaling, const float* row_keep, int vt_rows) -> int {
        QkvProj p;
        p.A = h;
        p.K = E;
        p.W = pk + a.wqkv;
        p.split = split_plan(m).qk;
        p.bias = (const float*)(pk + a.bqkv);
        p.q = q, p.k = k, p.vt = vt;
        p.cos = m->d_ucos;
        p.sin = m->d_usin;
        p.rows = N, p.T = T, p.Tp = Tp;
        p.scaling = scaling;
        p.row_keep = row_keep;
        p.vt_rows = vt_rows;
        GemmArgs g, gv;
        qkv_gemm_args(m, p, &g, &gv);
        if (s.weight_gemm(PC_GEMM_QKV, g, EPI_QKV_ROPE, os)) return 1;
        return s.weight_gemm(PC_GEMM_QKV, gv, EPI_V_T, os);
    };
    auto out_proj = [&](const AttnOff& a, int map_R, int map_C) -> int {
        GemmArgs g;
        g.A = h;
        g.W = pk + a.wo;
        g.bias = (const float*)(pk + a.bo);
        g.out = x;
        g.M = N;
        g.N = E;
        g.K = E;
        g.rowmap_R = map_R;
        g.rowmap_C = map_C;
        return s.weight_gemm(PC_GEMM_OUT, g, EPI_RESID_F32, 8);
    };

    for (int l = 0; l < L; ++l) {
        const MsaLayerOff& o = m->mlayer[l];
        // ---- tied row attention (axial_attention.py:75-130; NormalizedResidualBlock modules.py:376-392) ----
        if (s.lnorm(x, o.row.lng, o.row.lnb, h, nullptr, N, LnExtra())) return 1;
        if (Cp != C) ESMK_TRY(hipMemsetAsync(vt, 0, (size_t)B * H * R * 64 * Cp * os, st));
        // sequences = MSA rows (b,r) of C tokens; q scaled by d^-1/2 / sqrt(R) (axial_attention.py:36-38)
        if (qkv(o.row, C, Cp, (1.0f / sqrtf(64.0f)) / sqrtf((float)R), keep, R)) return 1;
        {   // scores[b,h,i,j] = sum_{r,d} q[r,i,b,h,d] k[r,j,b,h,d]   (axial_attention.py:90): K tile r of
            // the batched GEMM is the [C,64] matrix q[(b,r),h] (row stride 128 B)
            // slice s of MSA b is batch entry zo = b * S + s: R / S rows further down q / k, its own output map
            const int S = w.row_slices, Rs = R / S;
            GemmArgs g;
            g.A = q;
            g.W = k;
            g.out = scores;
            g.M = C;
            g.N = Cp;
            g.n_valid = C;
            g.K = Rs * 64;
            g.ldc = Cp;
            g.a_row_bytes = g.w_row_bytes = 128;
            g.a_kt_bytes = g.w_kt_bytes = (long long)H * C * 64 * os;
            g.batch = B * S * H;
            g.batch_inner = H;
            g.a_bo = g.w_bo = (long long)Rs * H * C * 64 * os;
            g.a_bi = g.w_bi = (long long)C * 64 * os;
            g.o_bo = (long long)H * C * Cp * 4;
            g.o_bi = (long long)C * Cp * 4;
            if (s.gemm(PC_MSA_ROW_SCORES, g, EPI_STORE_F32, 4)) return 1;
        }
        {
            const double sc = (double)B * H * C * C;
            ProfScope ps(m, st, PC_MSA_ROW_SOFTMAX, 0, sc * (4 + os + (want_attn ? 4 : 0)));
            ESMK_TRY(launch_msa_row_softmax(scores, keep, any_pad, probs,
                                            want_attn ? (float*)row_attn_out_dev : nullptr, B, H, R, C, Cp, l, L, op,
                                            st, w.row_slices));
        }
        {   // context[r,i,b,h,:] = sum_j probs[h,b,i,j] v[r,j,b,h,:]   (axial_attention.py:111)
            GemmArgs g;
            g.A = probs;
            g.W = vt;
            g.out = h;
            g.M = C;
            g.N = R * 64;
            g.K = Cp;
            g.ldc = E;
            g.a_row_bytes = g.w_row_bytes = (long long)Cp * os;
            g.batch = B * H;
            g.batch_inner = H;
            g.a_bo = (long long)H * C * Cp * os;
            g.a_bi = (long long)C * Cp * os;
            g.w_bo = (long long)H * R * 64 * Cp * os;
            g.w_bi = (long long)R * 64 * Cp * os;
            g.ctx_R = R;
            g.ctx_C = C;
            if (s.gemm(PC_MSA_ROW_CTX, g, EPI_MSA_CTX, os)) return 1;
        }
        if (out_proj(o.row, 0, 0)) return 1;

        // ---- column attention (axial_attention.py:185-239): every MSA column (b,c) is a sequence of R rows;
        // the normalised rows are written in (b,c,r) order so the ESM-2 attention path applies unchanged ----
        {
            LnExtra ex;
            ex.map_R = R;
            ex.map_C = C;
            if (s.lnorm(x, o.col.lng, o.col.lnb, h, nullptr, N, ex)) return 1;
        }
        if (Rp != R) ESMK_TRY(hipMemsetAsync(vt, 0, (size_t)B * C * H * 64 * Rp * os, st));
        // log2(e) folded into the q scale: the flash / map kernels work on log2-domain scores (attention.hip)
        if (qkv(o.col, R, Rp, kLog2e / sqrtf(64.0f), nullptr, 0)) return 1;
        float* lse = want_col ? (float*)(ws + w.lse) : nullptr;
        {
            ProfScope ps(m, st, PC_MSA_COL_ATTN, 4.0 * N * (double)R * E, 4 * NE * os);
            ESMK_TRY(launch_attention_fill(q, k, vt, col_fill, any_pad, h, lse, B * C, H, R, Rp, op, st));
        }
        if (want_col) {
            ProfScope ps(m, st, PC_ATTN_PROBS, 2.0 * N * (double)R * E, 2 * NE * os + 4.0 * N * R * H);
            ESMK_TRY(launch_attention_probs_msa(q, k, lse, col_fill, any_pad, (float*)col_attn_out_dev, B, C, H, R, l,
                                                L, op, st));
        }
        if (out_proj(o.col, R, C)) return 1;

        // ---- feed forward (modules.py:395-418) ----
        if (s.lnorm(x, o.flng, o.flnb, h, nullptr, N, LnExtra())) return 1;
        {
            GemmArgs g;
            g.A = h;
            g.W = pk + o.w1;
            g.bias = (const float*)(pk + o.b1);
            g.out = ffn;
            g.M = N;
            g.N = F;
            g.K = E;
            if (s.weight_gemm(PC_GEMM_FC1, g, EPI_GELU_T, os)) return 1;
            g = GemmArgs();
            g.A = ffn;
            g.W = pk + o.w2;
            g.bias = (const float*)(pk + o.b2);
            g.out = x;
            g.M = N;
            g.N = E;
            g.K = F;
            if (s.weight_gemm(PC_GEMM_FC2, g, EPI_RESID_F32, 8)) return 1;
        }
        if (l + 1 < L && s.repr_copy(l + 1, x)) return 1;  // msa_transformer.py:197-198
    }

    // msa_transformer.py:200-206: final LayerNorm (representation L is the normalised stream), LM head
    // The head runs on the rows it is asked for: all N of them, or (rows entry) the selection gathered out of the final stream.
    // Every kernel of the head computes a row from that row alone: a selected row carries the bits esmk_msa_forward gives it.
    if (const MsaRowSel* rs = c.rs) {
        const int rows = rs->n_sel;
        float* rx = (float*)(ws + rs->x);
        {
            ProfScope ps(m, st, PC_COPY, 0, 8.0 * rows * E);
            ESMK_TRY(launch_gather_rows(x, rs->sel_dev, rx, N, E, rows, st));
        }
        if (lm_head(s, rows, rx, ws + rs->h, (float*)(ws + rs->g32), E, LnExtra(), false, true, c.logits)) return 1;
        // torch.log_softmax(logits, dim=-1) of the selected rows (counted under "lm_head_logits", the gather under "repr_copy")
        ProfScope ps(m, st, PC_LM_LOGITS, 0, 8.0 * rows * m->V);
        ESMK_TRY(launch_log_softmax_rows((const float*)c.logits, rs->logprobs_out, nullptr, nullptr, rows, m->V, st));
        return 0;
    }
    if (lm_head(s, N, x, h, g32, E, LnExtra(), false, want_logits, c.logits)) return 1;
    if (want_contacts) {  // msa_transformer.py:215-217 -> modules.py:338-357 on the row attentions
        // the contact head reads tokens only for the <eos> mask, which the MSA alphabet does not append
        ProfScope ps(m, st, PC_CONTACTS, 0, 2.0 * 4 * B * (double)L * H * C * C);
        ESMK_TRY(launch_contacts((const float*)row_attn_out_dev, tokens_dev, (const float*)(pk + m->ct_w),
                                 (const float*)(pk + m->ct_b), (float*)(ws + w.ct_scratch),
                                 (float*)contacts_out_dev, B, L * H, C, m->cfg.eos_idx, m->cfg.prepend_bos,
                                 m->cfg.append_eos, st));
    }
    return 0;
}

}  // namespace
