// engine_internal.h — state and launch helpers shared by the host-side translation units of libesmk.so (engine.hip: ESM-2 /
// ESM-1b / ESM-1 path and the generic C ABI; engine_msa.hip: MSA Transformer path; engine_ops.hip: single-kernel and debug
// entries).  Not part of the public ABI.
#pragma once
#include "../../include/esmk.h"
#include "kernels.h"

#include <string>
#include <vector>

namespace esmk_host {

// error reporting: message kept per thread for esmk_last_error()
int fail(const char* what, hipError_t e);
int fail(const std::string& msg);

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
inline size_t op_size(int dt) { return dt == esmk::ESMK_DT_F32 ? 4 : 2; }

// sequential carving of byte offsets (256-byte aligned) out of one buffer
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes);
        return o;
    }
};

// packed-parameter offsets of one TransformerLayer (reference esm/modules.py:84-142)
struct LayerOff {
    size_t wqkv, bqkv, wo, bo, w1, b1, w2, b2, ln1g, ln1b, ln2g, ln2b;
    size_t bqkv2 = 0, b12 = 0;  // LayerNorm fold: W . beta of the folded q/k/v and fc1 weights (GemmArgs::bias2)
    size_t bkv = 0;             // ESM-1: self_attn.bias_k | bias_v, [H,64] each, operand dtype
};
// one AxialTransformerLayer (reference esm/modules.py:145-221)
struct AttnOff {
    size_t wqkv, bqkv, wo, bo, lng, lnb;
};
struct MsaLayerOff {
    AttnOff row, col;
    size_t w1, b1, w2, b2, flng, flnb;
};

}  // namespace esmk_host

// row counts travel as int through the kernels (row * ld products are widened to 64 bit); 2^24 rows of fp32
// residual already exceed one GPU's HBM for every supported width, so this is a guard, not a limit in practice.
// tests/test_index_width_ops_gpu.py and tests/test_index_width_engine_gpu.py run the kernels past 2^31 and 2^32 bytes.
#define ESMK_MAX_ROWS (1LL << 24)

#define ESMK_TRY(expr)                                             \
    do {                                                           \
        hipError_t _e = (expr);                                    \
        if (_e != hipSuccess) return esmk_host::fail(#expr, _e);   \
    } while (0)

struct esmk_model {
    esmk_config cfg;
    int L, E, H, F, V, D;
    int EA = 0;  // attention width inside the engine: H * 64 (heads with head_dim < 64 are spread over 64 slots)
    int Kp = 0;  // E rounded up to the 64-wide K tile: row stride of the normalised activations
    // packed parameter image layout (byte offsets)
    size_t embed_f32, embed_op, fin_g, fin_b, lm_w, lm_b, lm_lng, lm_lnb, lm_bias, ct_w, ct_b;
    size_t lm_w32 = 0;  // f16x2 precision mode: lm_head.dense.weight in fp32 (the head runs on the fp32 MFMA path)
    std::vector<esmk_host::LayerOff> layer;
    size_t packed_bytes;
    // RoPE
    std::vector<float> inv_freq;
    float* d_inv_freq = nullptr;
    float* d_cos = nullptr;
    float* d_sin = nullptr;
    int rope_cap = 0;
    // optional per-kernel-class timing with HIP events (esmk_profile_begin / _end)
    struct ProfRec {
        int cls;
        hipEvent_t a, b;
        double flops, bytes;
    };
    bool prof_on = false;
    std::vector<ProfRec> prof;
    // esmk_forward_packed: pinned host staging of the segment / work tables; pk_event = its last upload
    int32_t* pk_host = nullptr;
    size_t pk_host_cap = 0;
    hipEvent_t pk_event = nullptr;
    // LayerNorm fold: q/k/v and fc1 weights are packed gamma-folded and row-centred, the per-layer
    // LayerNorm passes become GEMM epilogue work.  fold_state[l]: bits of FoldBits — which inputs of the fold have been
    // packed, and which folded images are current (a LayerNorm parameter packed after its weights makes them stale).
    bool fold = false;
    std::vector<uint32_t> fold_state;
    // the packed image fold_state describes: the bits belong to ONE caller-owned image, so packing into (or running
    // on) another image starts from "nothing packed" instead of inheriting the previous image's bits
    const void* fold_image = nullptr;
    // MSA Transformer (esmk_msa_create)
    bool is_msa = false;
    int npos = 0, has_msa_pos = 0;
    size_t pos_emb = 0, msa_pos = 0, lnb_g = 0, lnb_b = 0;
    std::vector<esmk_host::MsaLayerOff> mlayer;
    // ESM-1 (esmk_config::no_rope = ESMK_ESM1 [| ESMK_ESM1_FINAL_BIAS]): embed_out [V,Kp] operand dtype, embed_out_bias [V] fp32; the sinusoidal table [sinus_cap, E]
    int esm1 = 0, final_bias = 0;
    size_t out_w = 0, out_b = 0;
    float* d_sinus = nullptr;
    int sinus_cap = 0;
    float* d_ucos = nullptr;  // "unit" rotary tables (cos = 1, sin = 0): the MSA model has no RoPE
    float* d_usin = nullptr;
    int unit_cap = 0;
    // edits of the residual stream between layers (esmk_set_stream_edits): copied descriptors, borrowed device pointers
    std::vector<esmk_stream_edit> edits;
    // early exit (esmk_set_layer_limit): 0 < layer_limit < L stops the forward after that many layers; 0: the whole stack
    int layer_limit = 0;
    // linear pairwise head on the attention maps (esmk_set_pair_head): device copies, w64 [L*H][64] (columns past the head's
    // outputs zero), bias [n_sym + n_asym]; both counts 0: no head
    float* d_pair_w64 = nullptr;
    float* d_pair_bias = nullptr;
    int pair_sym = 0, pair_asym = 0;
};

// Precision modes with split weights (esmk_config::weight_split): which matrices of a layer are kept as W_hi + W_lo (factor 2:
// image rows of 2 K, two MFMA passes) — 1 = f16x2: all;  2 = f16x2a: the attention projections q, k, v, out (a third of the
// GEMM work);  3 = f16x2v: the value path v, out only (a sixth of the GEMM work, most of f16x2a's accuracy: DESIGN.md I.2);
// 4 = f16x3: every matrix as hi | lo | hi (factor 3) against ACTIVATIONS laid out hi | hi | lo — weights and GEMM inputs both
// to ~20 bits: the mode that holds 1e-3 on every output, contact logits included
struct SplitPlan {
    int qk, v, o, ffn;
};
static inline SplitPlan split_plan(const esmk_model* m) {
    switch (m->cfg.weight_split) {
        case 1: return {2, 2, 2, 2};
        case 2: return {2, 2, 2, 1};
        case 3: return {1, 2, 2, 1};
        case 4: return {3, 3, 3, 3};
        default: return {1, 1, 1, 1};
    }
}
static inline bool split_x3(const esmk_model* m) { return m->cfg.weight_split == 4; }
// factor of one layer GEMM by its profiler class and epilogue (the v projection is the EPI_V_T launch of class PC_GEMM_QKV)
static inline int split_factor(const esmk_model* m, int cls, int epi);

// ---- per-kernel-class timing (esmk_profile_begin / _end): classes of both engines ---------------------------
enum {
    PC_EMBED = 0, PC_LAYERNORM, PC_GEMM_QKV, PC_ATTENTION, PC_ATTN_PROBS, PC_GEMM_OUT, PC_GEMM_FC1,
    PC_GEMM_FC2, PC_COPY, PC_LM_DENSE, PC_LM_LOGITS, PC_CONTACTS,
    PC_MSA_ROW_SCORES, PC_MSA_ROW_SOFTMAX, PC_MSA_ROW_CTX, PC_MSA_COL_ATTN, PC_LN_STATS, PC_STREAM_EDIT, PC_COUNT
};
static const char* const kProfNames[PC_COUNT] = {
    "embed", "layernorm", "gemm_qkv_rope", "attention", "attention_probs", "gemm_out_proj",
    "gemm_fc1_gelu", "gemm_fc2", "repr_copy", "lm_head_dense", "lm_head_logits", "contacts",
    "msa_row_scores", "msa_row_softmax", "msa_row_context", "msa_col_attention",
    // LayerNorm fold: the row-statistics entry pass and the per-LayerNorm finalize launches (tiny; the LayerNorm passes
    // themselves are GEMM epilogue work) — "layernorm" keeps the standalone LayerNorm kernel (with the fold: the final one)
    "ln_fold_stats",
    // edits of the stream between layers (interventions.hip): no record unless edits are set
    "stream_edit"};

static inline int split_factor(const esmk_model* m, int cls, int epi) {
    const SplitPlan s = split_plan(m);
    if (cls == PC_GEMM_QKV) return epi == esmk::EPI_V_T ? s.v : s.qk;
    if (cls == PC_GEMM_OUT) return s.o;
    return s.ffn;
}

// Brackets one launch with two events on the launch stream when profiling is enabled.
struct ProfScope {
    esmk_model* m;
    hipStream_t st;
    bool on;
    ProfScope(esmk_model* m_, hipStream_t st_, int cls, double flops, double bytes)
        : m(m_), st(st_), on(m_->prof_on) {
        if (!on) return;
        esmk_model::ProfRec r{cls, nullptr, nullptr, flops, bytes};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
            on = false;
            return;
        }
        (void)hipEventRecord(r.a, st);
        m->prof.push_back(r);
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(m->prof.back().b, st);
    }
};

enum FoldBits : uint32_t {
    FB_LN1G = 1, FB_LN1B = 2, FB_LN2G = 4, FB_LN2B = 8, FB_WQ = 16, FB_WK = 32, FB_WV = 64, FB_W1 = 128,
    FB_ALL_W = FB_WQ | FB_WK | FB_WV | FB_W1
};

namespace esmk_host {
constexpr float kLog2e = 1.4426950408889634f;
// head width inside the engine: 128, or 64 slots (heads with head_dim < 64 are spread over them)
inline int head_slots(const esmk_model* m) { return m->D == 128 ? 128 : 64; }

// esmk_debug_set("rows_contacts_own_groups", 1): esmk_forward_rows_contacts takes the batch's own head-group count instead of
// the pinned one — the measurement of what the pin costs (tools/design_throughput.py); process wide, off by default
extern int g_rows_contacts_own_groups;
// one edit descriptor against a stream of width E and, for the handle's list, a stack of L layers (L < 0: the single op, which
// has no layer); everything that needs no HIP call (engine.hip)
int check_stream_edit(const std::string& who, const esmk_stream_edit& e, int E, int L);
// the launch arguments of a descriptor on the stream x [N, E]; the fold outputs are the caller's to add
inline esmk::StreamEditArgs stream_edit_args(const esmk_stream_edit& e, float* x, const int64_t* tokens, int N, int E) {
    esmk::StreamEditArgs a;
    a.x = x, a.tokens = tokens, a.N = N, a.E = E;
    a.rows = e.rows_dev, a.n_rows = e.n_rows, a.token_set = e.token_set;
    a.src = e.src_dev, a.src_ld = e.src_ld, a.n_src = e.n_src, a.src_index = e.src_index_dev;
    a.keep = e.keep, a.gain = e.gain, a.op = e.op;
    return a;
}
// rotary tables for rows 0 .. T-1 (engine.hip)
int ensure_rope(esmk_model* m, int T, hipStream_t st);
// "unit" rotary tables (cos = 1, sin = 0) for models without RoPE (MSA Transformer, ESM-1b)
int ensure_unit_rope(esmk_model* m, int T, hipStream_t st);
// packed image layout of the MSA Transformer (engine_msa.hip)
void plan_packed_msa(esmk_model* m);

// ---- host launch helpers of both engines (engine.hip): one launch with its profiler record ------------------
struct Stack {
    esmk_model* m;
    hipStream_t st;
    int op;          // operand dtype
    size_t os;       // and its size
    const char* pk;  // packed parameter image
    int N;           // rows of the residual stream
    // requested representations (esmk_forward / esmk_msa_forward arguments)
    const int32_t* repr_layers;
    int n_repr;
    void* const* repr_out;

    void* repr_of(int layer) const {  // the first buffer that takes `layer`, or null
        for (int i = 0; i < n_repr; ++i)
            if (repr_layers[i] == layer) return repr_out[i];
        return nullptr;
    }
    // algorithmic work of one (batched) GEMM launch: operands read once, result written once (residual: read + written)
    int gemm(int cls, const esmk::GemmArgs& a, int epi, double out_bytes_per_elem) const;
    // a GEMM against a weight matrix of the layer stack: with split weights (f16x2) the same kernel runs over
    // the [N, 2K] hi | lo image, the activations' K tile kt / 2 meeting W_hi (kt even) and W_lo (kt odd); FLOP / byte
    // accounting stays algorithmic
    int weight_gemm(int cls, esmk::GemmArgs a, int epi, double out_bytes_per_elem) const;
    int lnorm(const float* in, size_t gamma_off, size_t beta_off, void* y, float* y32, int rows, const esmk::LnExtra& ex) const;
    // copies of the stream for every request of `layer`: fp32, or (lowp) the operand dtype
    int repr_copy(int layer, const float* src, bool lowp = false) const;
};
// Final LayerNorm (esm2.py:123-128: representation L is the normalised stream, fp32) and the LM head (modules.py:308-314) on
// `rows` rows of x; h, g32: operand-dtype and fp32 scratch rows.  With split weights the head runs in fp32 on the exact-fp32
// MFMA path.  repr_lowp: representations leave in the operand dtype — the caller has then run the final LayerNorm itself
// if layer L was requested.
int lm_head(const Stack& s, int rows, float* x, void* h, float* g32, int Kp, const esmk::LnExtra& ex, bool repr_lowp,
            bool want_logits, void* logits_out);

// The q / k (EPI_QKV_ROPE) and v (EPI_V_T) projections of one attention block: what differs between their callers
struct QkvProj {
    const void* A = nullptr;  // operand rows, K columns each (3 Kp in the f16x3 mode)
    int K = 0;
    const void* W = nullptr;  // q | k | v weight rows; the v rows start behind 2 EA rows of `split` * Kp elements
    int split = 1;
    const float *bias = nullptr, *bias2 = nullptr, *ln_rstd = nullptr;
    void *q = nullptr, *k = nullptr, *vt = nullptr;
    const float *cos = nullptr, *sin = nullptr;
    int rows = 0, T = 0, Tp = 0;
    float scaling = 1.f;
    const int* row_pos = nullptr;      // token-packed batches
    const float* row_keep = nullptr;   // MSA row attention
    int vt_rows = 0;
};
void qkv_gemm_args(const esmk_model* m, const QkvProj& p, esmk::GemmArgs* qk, esmk::GemmArgs* v);

// ---- token-packed row spaces: the segment table and the int32 tables behind the workspace -------------------
// The segment table of a packed row space, shared by the engine entries and the single-kernel entries: the layout rules,
// and the tables every packed attention launch reads.  lead_gap: the first segment may start behind row 0 (op entries).
struct SegTableInfo {
    int max_len = 0;
    size_t items = 0;                // 128-query blocks = entries of the attention work list
    unsigned long long sum_len2 = 0;
};
int check_seg_table(const std::string& w, const int32_t* seg, int n_seg, int rows, bool lead_gap, SegTableInfo* info);
// dst: [seg 2 n][npad n (zero: filled on the device)][work 4 items] — query blocks of 128 rows, longest segments first
void fill_attn_tables(const int32_t* seg, int n_seg, int32_t* dst);
// dst: uint64 [n_seg] (as int32 pairs, 8-byte aligned): map offset of segment s = sum of len^2 of the segments in front
void fill_map_offsets(const int32_t* seg, int n_seg, int32_t* dst);
// The one layout of that table, in int32 slots: [seg 2n][npad n][work 4 items][pad][contact tables (kernels.h,
// CtPackedPlan)][pad][map offsets uint64 n] — the contact tables and the map offsets 8-byte aligned, each only if asked for
struct PackedTables {
    size_t npad, work, ct_base, map_base, ints;
};
inline PackedTables packed_tables(int n_seg, size_t items, size_t ct_table_ints, bool maps) {
    PackedTables t;
    t.npad = (size_t)2 * n_seg;
    t.work = (size_t)3 * n_seg;
    const size_t lists = t.work + 4 * items;
    t.ct_base = (lists + 1) & ~(size_t)1;
    const size_t end = ct_table_ints ? t.ct_base + ct_table_ints : lists;
    t.map_base = (end + 1) & ~(size_t)1;
    t.ints = maps ? t.map_base + 2 * (size_t)n_seg : end;
    return t;
}
}  // namespace esmk_host
