/*
 * esmk.h — C ABI of libesmk.so, the MI355X (gfx950) ESM-2 forward engine.
 *
 * The reference (facebookresearch/esm) has no FFI: its boundary for this path is the Python
 * call  ESM2.forward(tokens, repr_layers, need_head_weights, return_contacts)
 * (reference esm/model/esm2.py:77-147).  libesmk.so sits directly under that call: the Python
 * class esm_amd.esm2.ESM2 keeps the reference's nn.Module surface and hands raw device
 * pointers to esmk_forward().  Every entry point below names the reference code it replaces.
 *
 * Conventions
 *   - every pointer named *_dev is a device pointer owned by the caller (a torch tensor);
 *     the library borrows it for the duration of the call and allocates nothing persistent
 *     except the small RoPE cos/sin table (freed in esmk_destroy);
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value 0 = ok, non-zero = error, message via esmk_last_error() (thread local);
 *   - a handle is bound to the device that was current at esmk_create() and is not re-entrant.
 */
#ifndef ESMK_H
#define ESMK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types for esmk_bind_weight / operand_dtype */
enum { ESMK_F32 = 0, ESMK_F16 = 1, ESMK_BF16 = 2 };

/* esmk_forward out_flags */
enum {
    ESMK_OUT_LOGITS = 1u,   /* logits [B,T,V] fp32                       (esm2.py:129)      */
    ESMK_OUT_ATTN = 2u,     /* attentions [B,L,H,T,T] fp32               (esm2.py:132-139)  */
    ESMK_OUT_CONTACTS = 4u, /* contacts [B,T-2,T-2] fp32                 (esm2.py:140-142).  Together with
                               ESMK_OUT_ATTN: computed from the attention tensor like the reference
                               (modules.py:338-357).  WITHOUT ESMK_OUT_ATTN (predict_contacts, esm2.py:146-147):
                               accumulated layer by layer, no [B,L,H,T,T] tensor exists (csrc/contacts.hip)        */
    ESMK_OUT_COL_ATTN = 8u, /* esmk_msa_forward: col_attentions [B,L,H,C,R,R] fp32 (msa_transformer.py:193-194) */
    /* `.half()` / `.bfloat16()` models return their outputs in the model dtype (esm2.py:77-144 run under
     * nn.Module.half(); ESMFold's language-model front end does exactly that, esmfold/v1/esmfold.py:61-67,118-135,
     * and stacks all L+1 representations).  With these flags the engine writes them in the OPERAND dtype directly
     * instead of fp32 + a cast pass: */
    ESMK_OUT_REPR_LOWP = 16u, /* repr_out_dev[i] are operand-dtype [B,T,E] (esmk_forward and esmk_forward_packed) */
    ESMK_OUT_ATTN_LOWP = 32u  /* attn_out_dev is operand-dtype [B,L,H,T,T]; not together with ESMK_OUT_CONTACTS on
                                 the materialised path (the contact kernels read fp32 maps) */
};

typedef struct esmk_model esmk_model;

/* Model hyper-parameters: the constructor arguments of ESM2 (esm/model/esm2.py:15-38) plus the
 * alphabet ids it copies from the Alphabet (esm/data.py:116-120). */
/* esmk_config::no_rope values above 1: the original ESM-1 models (arch "protein_bert_base", reference
 * esm/model/esm1.py:107-114).  They ride in this field because the struct has no size field and its layout is pinned
 * (18 int32_t = 72 bytes): a caller built against it keeps working, and 0 / 1 keep their meaning.
 * ESMK_ESM1: token embedding x sqrt(embed_dim); sinusoidal positions (sin | cos halves, position pad_idx + 1 + t, pads take
 * the zero row; the table is built by the engine) instead of a learned table; no embedding LayerNorm and no pad zeroing;
 * LayerNorm eps 1e-12; every attention layer has one learned null key / value pair (packed keys
 * layers.N.self_attn.bias_k / bias_v, [1,1,E]; never masked); no final LayerNorm — representation num_layers is the raw
 * stream — and logits = x . embed_out^T (packed key embed_out [vocab,E]).  Attention maps drop the null key's column (rows sum
 * to less than 1), as the reference returns them.
 * ESMK_ESM1_FINAL_BIAS (only together with ESMK_ESM1): args.final_bias — embed_out_bias [vocab] is added to the logits.
 * Needs head_dim 64, weight_split 0, num_positions 0, ln_before 0; the LayerNorm fold does not exist for these models
 * (ln_fold 0 resolves to off, ln_fold 1 fails) and neither does the token-packed form (esmk_forward_packed* fail). */
#define ESMK_ESM1 2
#define ESMK_ESM1_FINAL_BIAS 4

typedef struct esmk_config {
    int32_t num_layers;      /* L                                                        */
    int32_t embed_dim;       /* E                                                        */
    int32_t num_heads;       /* H, head_dim d = E/H                                      */
    int32_t ffn_dim;         /* 4E for ESM-2 (esm2.py:53)                                */
    int32_t vocab;           /* len(alphabet) = 33                                       */
    int32_t pad_idx, mask_idx, cls_idx, eos_idx;
    int32_t token_dropout;   /* esm2.py:86-92                                            */
    int32_t prepend_bos, append_eos; /* contact head crop (modules.py:338-347)           */
    int32_t operand_dtype;   /* ESMK_F16 or ESMK_BF16: MFMA operand type; accumulation,
                                residual stream, LayerNorm, softmax are always fp32     */
    /* ESM-1b / ESM-1v (ProteinBertModel with arch "roberta_large", esm/model/esm1.py:88-104,117-143); all
     * zero for ESM-2 */
    int32_t no_rope;         /* 1: no rotary embedding (TransformerLayer(use_rotary_embeddings=False));
                                ESMK_ESM1 (2), or ESMK_ESM1 | ESMK_ESM1_FINAL_BIAS (6): the original ESM-1 architecture, see
                                above (no rotary embedding either)                                     */
    int32_t num_positions;   /* > 0: rows of the LearnedPositionalEmbedding table added to the token embedding
                                (esm1.py:133, modules.py:240-257); key "embed_positions.weight"   */
    int32_t ln_before;       /* 1: emb_layer_norm_before (esm1.py:136-137)                          */
    /* Precision mode "f16x2" (operand_dtype must be ESMK_F16): the weight matrices of the layer stack are kept as
     * W = W_hi + W_lo (two fp16 images, ~20 bits of every weight) and every layer GEMM runs both against the fp16
     * activations — the weight rounding, two thirds of the fp16-operand error of a 33-layer stack,
     * disappears at 2x the GEMM time.  Parameter image 2x larger.  0 = plain fp16 / bf16 operands.
     * 2 = "f16x2a" (round 6): the same for the ATTENTION projections only (q, k, v, out_proj:
     * esm/multihead_attention.py:256-261,395 — a third of the GEMM work); fc1 / fc2 stay plain fp16, the LM head runs in
     * fp32 as with 1.  Representations and logits inside 1e-3 in both norms at ~1.3x the plain step.
     * 3 = "f16x2v": the value path only (v_proj, out_proj: a sixth of the GEMM work, ~1.2x).
     * 4 = "f16x3": weights AND GEMM inputs split — every matrix is packed hi | lo | hi per 64-column K tile and every layer
     * GEMM runs as a plain launch over K' = 3 K on operand rows hi | hi | lo (A_hi W_hi + A_hi W_lo + A_lo W_hi); only q / k, v
     * and P of the attention stay fp16.  Representations, logits AND contact logits inside 1e-3 of the reference
     * (tests/test_readme.py:116 atol) at ~2.4x the step.  head_dim 64, embed_dim % 64 == 0, padded batches (esmk_forward). */
    int32_t weight_split;
    /* LayerNorm fold (reference esm/modules.py:120-140, the two LayerNorm -> Linear pairs of a TransformerLayer): 1 = the
     * q/k/v and fc1 weights are packed multiplied by the LayerNorm weight and row-centred, the residual GEMMs emit the
     * operand-dtype rows and their statistics, and the standalone per-layer LayerNorm passes disappear (plain fp16 / bf16
     * operands, head_dim <= 64; esmk_create fails otherwise); -1 = off; 0 = the library's default (environment
     * ESMK_LN_FOLD=0|1 overrides it).  With the fold the LayerNorm weight and bias of a layer MUST be packed before
     * that layer's q/k/v and fc1 weights (esmk_pack_weight fails otherwise; esmk_forward fails while a fold is stale).
     * The handle tracks the fold of ONE packed image at a time — the one esmk_pack_weight last wrote to; packing into a
     * different image starts from "nothing packed", and esmk_forward refuses an image the handle did not pack.
     * Library default since round 5: ON. */
    int32_t ln_fold;
} esmk_config;

const char* esmk_last_error(void);
const char* esmk_version(void);

/* Replaces ESM2.__init__/_init_submodules (esm2.py:15-75): records dimensions only. */
int esmk_create(const esmk_config* cfg, esmk_model** out);
void esmk_destroy(esmk_model* m);

/* RoPE inverse frequencies, fp32 host array of head_dim/2 values, exactly the buffer
 * RotaryEmbedding.__init__ builds (esm/rotary_embedding.py:40-41). The cos/sin tables
 * (rotary_embedding.py:47-61) are built on the device in fp32 from it. */
int esmk_set_rope_inv_freq(esmk_model* m, const float* inv_freq_host, int n);

/* Bytes of the packed parameter image (operand-dtype matrices + fp32 vectors). */
int esmk_packed_bytes(const esmk_model* m, size_t* bytes);

/* Replaces nn.Module.load_state_dict for the engine copy: converts ONE state-dict tensor
 * (key names as in esm2.py state_dict, e.g. "layers.3.self_attn.q_proj.weight") from its
 * device buffer into the packed image.  q/k/v projections are concatenated to one [3E,E]
 * operand; the tied lm_head.weight (esm2.py:71-75) is taken from embed_tokens.weight.
 * Unknown keys (e.g. "...rot_emb.inv_freq") return 0 and are ignored. */
int esmk_pack_weight(esmk_model* m, void* packed_dev, size_t packed_bytes, const char* key,
                     const void* src_dev, int src_dtype, const int64_t* shape, int ndim,
                     void* stream);

/* Workspace bytes for one forward of [B,T] tokens with the given outputs. */
int esmk_workspace_bytes(const esmk_model* m, int B, int T, uint32_t out_flags, size_t* bytes);

/* Replaces ESM2.forward (esm/model/esm2.py:77-144) — embedding + token dropout, the
 * TransformerLayer loop (esm/modules.py:120-142 -> esm/multihead_attention.py:159-405,
 * esm/rotary_embedding.py:63-69), final LayerNorm, RobertaLMHead (modules.py:308-314),
 * attention maps and ContactPredictionHead (modules.py:338-357).
 *   tokens_dev     int64 [B,T]
 *   repr_layers    host array of n_repr layer indices in [0,L]; repr_out_dev[i] fp32 [B,T,E]
 *   logits_out_dev fp32 [B,T,V]            (required iff ESMK_OUT_LOGITS)
 *   attn_out_dev   fp32 [B,L,H,T,T]        (required iff ESMK_OUT_ATTN)
 *   contacts_out_dev fp32 [B,T-2,T-2]      (required iff ESMK_OUT_CONTACTS)
 */
int esmk_forward(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                 const int32_t* repr_layers, int n_repr, void* const* repr_out_dev,
                 uint32_t out_flags, void* logits_out_dev, void* attn_out_dev,
                 void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes,
                 void* stream);

/* ---- token-packed batches: the same forward without compute on padding -------------
 * The reference pads every batch to its longest member (esm/data.py:269-277) and ESM2.forward computes the
 * pad rows (esm2.py:94-95 only zeroes them at the input).  Here the caller lays the sequences of a batch back
 * to back in ONE row space of `rows` rows (rows % 64 == 0): segment s occupies rows
 * [segments_host[2s], segments_host[2s] + segments_host[2s+1]); segment 0 starts at row 0, starts are
 * ascending multiples of 16, rows between segments ("gaps") hold pad_idx.  Every token attends to its own
 * segment only, rotary positions restart at each segment, the token-dropout ratio (esm2.py:86-92) is per
 * segment: rows of a segment carry exactly the values esmk_forward gives that sequence alone.
 *   tokens_dev      int64 [rows]
 *   segments_host   int32 [n_seg][2] on the HOST (first row, length incl. <cls>/<eos>)
 *   repr_out_dev[i] fp32 [rows,E]; logits_out_dev fp32 [rows,V] (iff ESMK_OUT_LOGITS); gap rows are undefined
 * ESM-1b / ESM-1v handles work the same way (learned positions restart at each segment, esm/modules.py:240-257).
 * esmk_packed_workspace_bytes / esmk_forward_packed refuse ESMK_OUT_ATTN and ESMK_OUT_CONTACTS: contacts of a packed
 * batch take the _ex entries below, attention maps (with or without contacts) the _maps entries behind them. */
int esmk_packed_workspace_bytes(const esmk_model* m, int n_seg, int rows, uint32_t out_flags, size_t* bytes);
int esmk_forward_packed(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                        const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers,
                        int n_repr, void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same with contact maps (ESMK_OUT_CONTACTS, predict_contacts' formula, no attention tensor): every segment's map
 * is the one esmk_forward(ESMK_OUT_CONTACTS) gives that sequence alone.  The workspace grows with sum(len^2) instead
 * of B*Tmax^2, so its size takes the segment table.  Accepted flags: ESMK_OUT_LOGITS (optional), ESMK_OUT_REPR_LOWP,
 * ESMK_OUT_CONTACTS; ESMK_OUT_ATTN / ESMK_OUT_ATTN_LOWP fail here (attention maps of a packed batch take the _maps
 * entries below), as does an MSA handle or the f16x3 precision mode.  Without ESMK_OUT_CONTACTS both behave as the entries above.
 *   contacts_out_dev fp32, ragged: with S_s = len_s - prepend_bos - append_eos, segment s's [S_s,S_s] map is row-major
 *                    at element offset sum_{s'<s} max(S_s',0)^2 (segments with S_s <= 0 have an empty map); required
 *                    iff ESMK_OUT_CONTACTS, even when every map is empty */
int esmk_packed_workspace_bytes_ex(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows,
                                   uint32_t out_flags, size_t* bytes);
int esmk_forward_packed_ex(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                           const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers,
                           int n_repr, void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev,
                           void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same with attention maps (need_head_weights=True: multihead_attention.py:396-403 per layer, stacked by
 * esm2.py:132-139), per sequence instead of per padded batch: no [B,L,H,Tmax,Tmax] tensor exists anywhere, neither in
 * the output nor in the workspace (which gains only the row log-sum-exp [H,rows] and the map offsets).
 * Accepted flags: ESMK_OUT_LOGITS, ESMK_OUT_REPR_LOWP, ESMK_OUT_CONTACTS, ESMK_OUT_ATTN (fp32 maps) and ESMK_OUT_ATTN_LOWP
 * (maps in the operand dtype; implies the maps, with or without ESMK_OUT_ATTN).  ESMK_OUT_CONTACTS is ALWAYS the fused
 * per-segment form of the _ex entries — also together with the map flags, unlike esmk_forward, which then derives the
 * contacts from the attention tensor; so ESMK_OUT_ATTN_LOWP and ESMK_OUT_CONTACTS combine freely here.  Without a map
 * flag both entries behave as the _ex entries.  ESM-1 (no_rope = ESMK_ESM1) handles, the f16x3 precision mode and MSA
 * handles are refused as there.
 *   attn_out_dev    ragged: segment s owns a contiguous row-major [L,H,len_s,len_s] block at element offset
 *                   L * H * sum_{s'<s} len_s'^2 (len includes <cls>/<eos>): exactly the [:, :, :len, :len] corner of that
 *                   sequence's slice of esmk_forward's padded tensor, bit for bit; rows / columns of <pad> tokens inside a
 *                   segment are zero.  fp32, or the operand dtype with ESMK_OUT_ATTN_LOWP.  Required iff a map flag is set.
 *   attn_out_elems  elements the buffer holds; checked against L * H * sum(len^2) before anything is launched (the
 *                   offsets pass 2^31 for ordinary batches, a short buffer would be written far out of bounds)
 *   contacts_out_dev as in esmk_forward_packed_ex */
int esmk_packed_workspace_bytes_maps(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows,
                                     uint32_t out_flags, size_t* bytes);
int esmk_forward_packed_maps(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev,
                             const int32_t* segments_host, int n_seg, int rows, const int32_t* repr_layers, int n_repr,
                             void* const* repr_out_dev, uint32_t out_flags, void* logits_out_dev, void* attn_out_dev,
                             size_t attn_out_elems, void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream);

/* ---- variant scoring: log-probabilities of selected rows (examples/variant-prediction/predict.py) -------
 * The reference scores a protein with one forward per masked position at B = 1, builds [1,T,V] logits each time and keeps
 * one row (predict.py:205-215, :138-143).  Here the caller runs those sequences as ONE padded batch and names the rows it
 * wants: the layer stack runs on all B*T rows; the final LayerNorm, the LM head (ESM-1: the embed_out GEMM; split-weight
 * modes: the fp32 head) and the vocabulary GEMM run on the n_sel selected rows only, and a log-softmax over the vocabulary
 * (torch.log_softmax(logits, dim=-1)) is written for exactly those rows.  No [B,T,V] tensor exists.  Every kernel of the
 * head computes a row from that row alone, so a selected row's logits are the bits esmk_forward gives that row.
 *   tokens_dev       int64 [B,T], padded as for esmk_forward
 *   sel_rows_dev     int32 [n_sel] on the DEVICE, flat row indices b*T + t in any order, repeats allowed.  Not validated on
 *                    the host: the gather clamps each index to [0, B*T), so a wrong index reads a valid row
 *   logprobs_out_dev fp32 [n_sel, V]
 *   workspace        esmk_rows_workspace_bytes(m, B, T, n_sel, &bytes, &logits_offset); after the call the selected logits
 *                    (fp32 [n_sel, V]) stay at byte offset *logits_offset of the workspace (logits_offset may be NULL)
 * vocab <= 64.  ESM-2, ESM-1b / ESM-1v and ESM-1 handles, with whatever operand dtype and precision mode esmk_forward runs
 * that handle in (the f16x3 mode keeps its restriction to head_dim-64 models here too); MSA handles are refused.  The whole
 * call runs on `stream`; error messages name esmk_forward_rows. */
int esmk_rows_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset);
int esmk_forward_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                      const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream);

/* ---- design toward a target contact map: selected log-prob rows AND contact maps in one forward ----------------
 * esmk_forward_rows plus ESMK_OUT_CONTACTS in the fused form (no [B,L,H,T,T] tensor): the layer stack runs once on all B*T rows,
 * the head of the model on the n_sel selected rows as in esmk_forward_rows (the same bits), and the contact head accumulates
 * contacts_out_dev fp32 [B,S,S] (S = T minus the <cls> / <eos> the alphabet adds) layer by layer.  It is the energy forward of
 * esm_amd/design.py: one call gives the LM term's rows and the structure term's maps of a batch of proposals.
 * The head-group pin: esmk_forward cuts the heads of a layer into a number of groups that it chooses from B (more groups where
 * few (query block, key chunk) pairs would leave compute units idle), and a map is the sum of the group accumulators in group
 * order — so the last bits of a sequence's map depend on the batch it runs in.  This entry always takes the group count of
 * B = 1: map b of the batch is bit for bit what esmk_forward(ESMK_OUT_CONTACTS) gives tokens[b] alone at B = 1, whatever B is, and
 * an acceptance test on an energy of that map makes the same decision alone and in any batch.  esmk_forward keeps its own
 * choice.  The price is workspace: the accumulators take G(1)*B*T*T*4 bytes where esmk_forward takes G(B) of them — up to
 * H*B*T*T*4 bytes (G(1) = min(H, ceil(1024 / ceil(T/128)^2)) for head_dim <= 64); ask esmk_rows_contacts_workspace_bytes, not
 * esmk_workspace_bytes.
 *   n_sel = 0 is allowed: no head runs, sel_rows_dev and logprobs_out_dev may be NULL (an energy with the contact term alone)
 *   logits_offset    as in esmk_rows_workspace_bytes (nothing is kept there with n_sel = 0)
 * ESM-2, ESM-1b / ESM-1v and ESM-1 handles (the fused contact head reads the bias_kv attention's q, k and row log-sum-exp like
 * any other), in whatever operand dtype and precision mode esmk_forward runs contacts for that handle.  Refused before any HIP
 * call: MSA handles, null pointers, B or T <= 0, B*T or n_sel > 2^24, n_sel < 0, vocab > 64 with n_sel > 0, a T that leaves no
 * residue (S <= 0), a workspace that is too small.  The whole call runs on `stream`; messages name esmk_forward_rows_contacts. */
int esmk_rows_contacts_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset);
int esmk_forward_rows_contacts(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                               const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, float* contacts_out_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
/* The head-group count of the fused contact head for a padded batch (no GPU needed): pinned 0 = esmk_forward at this B,
 * 1 = esmk_forward_rows_contacts (the count of B = 1, whatever B is). */
int esmk_debug_contact_groups(const esmk_model* m, int B, int T, int pinned, int32_t* groups);

/* Edits of the residual stream between layers: activation patching, steering, ablation — what a forward hook on
 * model.layers[k] that returns a changed output does to the reference.  The edits are state of the handle: while set, every
 * esmk_forward, esmk_forward_rows and esmk_forward_rows_contacts applies the edits of layer k, in list order, to the fp32
 * stream after k layers (k = 0: after the embedding, with the positions and emb_layer_norm_before of ESM-1b) and BEFORE
 * representation k is captured — repr_layers shows the edited stream — so every later layer and the head see it.  k = L
 * edits the stream in front of the final LayerNorm (ESM-1: the stream the output projection reads).  With the LayerNorm fold
 * an edited row of a layer 1 .. L-1 re-enters the fold's chain (operand row, mean, rstd) by esmk_op_rowstats' arithmetic.
 *   op ESMK_EDIT_AXPBY    x' = keep * x + gain * s, each product and the sum rounded to fp32 on its own (no fused
 *                         multiply-add); src_dev NULL: x' = keep * x.  set (0, 1), add (1, a), scale (a, no src), zero (0, no src)
 *   op ESMK_EDIT_PROJECT  c = gain <x, s> / <s, s>, both dot products accumulated in fp64, c rounded once to fp32;
 *                         x' = x - c * s (product and difference rounded on their own); <s, s> = 0: the row stays as it is
 *   rows_dev  int32 [n_rows], indices b*T + t into the call's B*T rows; indices outside are skipped; an index listed
 *             twice is the caller's error.  NULL: every row whose token is in token_set (bit v = token v; vocab <= 64)
 *   src_dev   fp32, n_src rows of stride src_ld: 0 (one vector for every row) or >= E, a multiple of 4; 16-byte aligned rows
 *   src_index_dev  int32, the source row of listed row i (of row r under the token selector); NULL: i (r).  A row whose
 *             source index is outside [0, n_src) is left as it is
 * The descriptors are copied; the device pointers are borrowed until the edits are cleared (n = 0) or replaced.  At most
 * ESMK_MAX_STREAM_EDITS.  Refused before any HIP call: an MSA handle, a layer outside [0, L], an unknown op, PROJECT
 * without src_dev, a bad src_ld, n_rows < 0, E > 5120; and, while edits are set, the token-packed entries
 * (esmk_forward_packed*, whose row space is not the caller's B*T rows).  With no edits set no launch, no workspace byte and
 * no output bit differs from a handle that never had any. */
enum { ESMK_EDIT_AXPBY = 0, ESMK_EDIT_PROJECT = 1 };
#define ESMK_MAX_STREAM_EDITS 64
typedef struct esmk_stream_edit {
    int32_t layer; /* 0..L: the stream after `layer` layers; 0 = the embedded stream */
    int32_t op;    /* ESMK_EDIT_AXPBY | ESMK_EDIT_PROJECT */
    float keep, gain;
    const int32_t* rows_dev; /* or NULL + token_set */
    int32_t n_rows;
    uint64_t token_set;
    const float* src_dev;
    int32_t src_ld;
    int32_t n_src;
    const int32_t* src_index_dev;
} esmk_stream_edit;
int esmk_set_stream_edits(esmk_model* m, const esmk_stream_edit* edits, int n);
/* Early exit: state of the handle, like the edits.  n_layers = 0 or L: the whole stack (the default; a fresh handle behaves as
 * before).  With 0 < n < L, esmk_forward, esmk_forward_packed and esmk_forward_packed_ex run the embedding stage, layers
 * 0 .. n - 1 with the stream edits and the representation copies of layers 0 .. n, and return: no final LayerNorm, no head, no
 * map and no contact stage.  Representation k <= n carries the bits the whole forward gives it.  With the LayerNorm fold the
 * last residual epilogue still emits the operand rows of layer n, which nothing reads.  Workspace sizes do not change.
 * Refused by name before any HIP call while such a limit is set: ESMK_OUT_LOGITS, ESMK_OUT_ATTN, ESMK_OUT_ATTN_LOWP,
 * ESMK_OUT_CONTACTS, a repr_layers entry above n, a held stream edit at a layer above n, and the entries esmk_forward_rows,
 * _rows_contacts, _rows_pair, _packed_rows and _packed_maps.  esmk_set_layer_limit itself refuses an MSA handle and n outside
 * 0 .. L (the limit that was set stays). */
int esmk_set_layer_limit(esmk_model* m, int n_layers);
/* One edit as a single op on x fp32 [N,E] in place (tokens_dev int64 [N], read under the token selector only), with the fold
 * outputs when y_dev is given: y[row][c] = T(x' - mean) (operand dtype, row stride ldy >= E; columns [E, ldy) are not
 * written), mean[row], rstd[row] — the bits esmk_op_rowstats gives on x'.  Rows that are not selected are neither read nor
 * written in any buffer.  E % 4 == 0, E <= 5120. */
int esmk_op_stream_edit(float* x_dev, const int64_t* tokens_dev, int N, int E, const esmk_stream_edit* edit, void* y_dev, int ldy,
                        float* mean_dev, float* rstd_dev, int operand_dtype, void* stream);

/* The same for a token-packed batch: the masked copies of a library of sequences of DIFFERENT lengths (pseudo-log-likelihood
 * of designed sequences, insertion / deletion variants, wt-marginals over a FASTA file) laid back to back in one row space,
 * so that the layer stack does no work on padding.  It is the reference's loop (predict.py:138-143,205-215: one B = 1 forward
 * per masked position, one row kept) for every sequence of the library at once: the layer stack of esmk_forward_packed on
 * the `rows` rows, the head of esmk_forward_rows on the n_sel selected ones.  Segment rules of esmk_forward_packed:
 * rows % 64 == 0, 0 < rows <= 2^24; segment s occupies rows [segments_host[2s], segments_host[2s] + segments_host[2s+1]);
 * segment 0 starts at row 0, starts are ascending multiples of 16, segments are disjoint with lengths > 0 inside `rows`;
 * rows between segments hold pad_idx.  Every segment carries the bits of that sequence alone, so a selected row's logits
 * and log-probabilities are bit for bit those esmk_forward_rows gives the same row of the same sequence in a padded batch.
 *   tokens_dev       int64 [rows] (esmk_op_mask_rows_packed builds it on the device)
 *   segments_host    int32 [n_seg][2] on the HOST (first row, length incl. <cls>/<eos>)
 *   sel_rows_dev     int32 [n_sel] on the DEVICE: flat row indices into the packed row space, any order, repeats allowed;
 *                    not validated on the host, the gather clamps each index to [0, rows)
 *   logprobs_out_dev fp32 [n_sel, V]
 *   workspace        esmk_packed_rows_workspace_bytes(m, segments_host, n_seg, rows, n_sel, &bytes, &logits_offset): the packed
 *                    forward's workspace, then the gathered rows, their operand rows, the head scratch and the selected
 *                    logits, which stay at byte offset *logits_offset (may be NULL) for the caller
 * vocab <= 64.  ESM-2 at every head_dim and ESM-1b / ESM-1v handles, plain and LayerNorm-fold, fp16 / bf16 and the f16x2
 * family.  MSA handles, ESM-1 (no_rope = ESMK_ESM1) handles and the f16x3 precision mode have no packed forward and are
 * refused before any HIP call.  The whole call runs on `stream`; error messages name esmk_forward_packed_rows. */
int esmk_packed_rows_workspace_bytes(const esmk_model* m, const int32_t* segments_host, int n_seg, int rows, int n_sel,
                                     size_t* bytes, size_t* logits_offset);
int esmk_forward_packed_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, const int32_t* segments_host,
                             int n_seg, int rows, const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- MSA Transformer (reference esm/model/msa_transformer.py:20-238, esm/axial_attention.py) -------- */

/* Constructor arguments of MSATransformer (msa_transformer.py:88-144) + alphabet ids. */
typedef struct esmk_msa_config {
    int32_t num_layers, embed_dim, num_heads, ffn_dim, vocab;
    int32_t pad_idx, mask_idx, cls_idx, eos_idx, prepend_bos, append_eos;
    int32_t num_positions;               /* rows of embed_positions.weight = max_positions + pad_idx + 1 */
    int32_t has_msa_position_embedding;  /* args.embed_positions_msa (msa_transformer.py:104-112) */
    int32_t operand_dtype;               /* ESMK_F16 or ESMK_BF16 */
    int32_t weight_split;                /* 1: precision mode f16x2 (see esmk_config::weight_split; operand_dtype ESMK_F16): every weight
                                            matrix of the axial layers as W_hi + W_lo, the LM head on the fp32 MFMA path;
                                            2: f16x2a, the row / column attention projections only; 3: f16x2v, their v / out
                                            projections only */
} esmk_msa_config;

/* Replaces MSATransformer.__init__; the handle is packed with esmk_pack_weight (MSATransformer
 * state-dict keys: layers.N.{row,column}_self_attention.layer.*_proj.*, ...layer_norm.*,
 * layers.N.feed_forward_layer.layer.fc{1,2}.*, embed_positions.weight, msa_position_embedding, ...)
 * and freed with esmk_destroy. */
int esmk_msa_create(const esmk_msa_config* cfg, esmk_model** out);
int esmk_msa_workspace_bytes(const esmk_model* m, int B, int R, int C, uint32_t out_flags, size_t* bytes);

/* Replaces MSATransformer.forward (msa_transformer.py:146-220): embedding (+ LearnedPositionalEmbedding
 * modules.py:240-257), AxialTransformerLayer stack (modules.py:196-221: RowSelfAttention
 * axial_attention.py:75-130, ColumnSelfAttention :185-239, FeedForwardNetwork modules.py:395-418),
 * final LayerNorm, RobertaLMHead, ContactPredictionHead on the row attentions.
 *   tokens_dev       int64 [B,R,C]
 *   repr_out_dev[i]  fp32 [B,R,C,E]
 *   logits_out_dev   fp32 [B,R,C,V]        (iff ESMK_OUT_LOGITS)
 *   row_attn_out_dev fp32 [B,L,H,C,C]      (iff ESMK_OUT_ATTN or ESMK_OUT_CONTACTS)
 *   col_attn_out_dev fp32 [B,L,H,C,R,R]    (iff ESMK_OUT_COL_ATTN; 4.8 GB per layer for a 128 x 513 MSA)
 *   contacts_out_dev fp32 [B,C-1,C-1]      (iff ESMK_OUT_CONTACTS) */
int esmk_msa_forward(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int R, int C,
                     const int32_t* repr_layers, int n_repr, void* const* repr_out_dev, uint32_t out_flags,
                     void* logits_out_dev, void* row_attn_out_dev, void* col_attn_out_dev,
                     void* contacts_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- variant scoring with the MSA Transformer: log-probabilities of selected rows (predict.py:161-184) -------
 * The reference masks position i of the first row of an MSA, runs one forward of the whole MSA per column at B = 1 and keeps
 * log_softmax(logits)[0, 0, i].  Here the caller runs the masked copies of the MSA as ONE batch [B,R,C] and names the rows it
 * wants, as esmk_forward_rows does for the single-sequence models: the layer stack of esmk_msa_forward runs on all B*R*C
 * rows; the final LayerNorm, the LM head and the vocabulary GEMM run on the n_sel selected rows only, and their log-softmax
 * is written.  No [B,R,C,V] tensor exists.
 *   tokens_dev       int64 [B,R,C]
 *   sel_rows_dev     int32 [n_sel] on the DEVICE, flat indices (b*R + r)*C + c in any order, repeats allowed.  Not validated
 *                    on the host: the gather clamps each index to [0, B*R*C), so a wrong index reads a valid row
 *   logprobs_out_dev fp32 [n_sel, V]
 *   workspace        esmk_msa_rows_workspace_bytes(m, B, R, C, n_sel, &bytes, &logits_offset); after the call the selected
 *                    logits (fp32 [n_sel, V]) stay at byte offset *logits_offset of the workspace (logits_offset may be NULL)
 * The slice pin: esmk_msa_forward cuts the tied-row score contraction over the R rows into a number of K slices that it
 * chooses from B (more slices where few output tiles would leave compute units idle), and the row softmax adds the partial
 * maps in slice order — so the summation order of a copy's scores depends on the batch it runs in.  This entry always takes
 * the slice count of B = 1 (its workspace holds the score maps of that count): copy b of the batch is computed with the
 * launches and the summation order of esmk_msa_forward at B = 1 on that copy, and a selected row carries the bits of that
 * forward whatever B is.  esmk_msa_forward keeps its own choice.  The guarantee is for a batch of masked copies of ONE MSA
 * (the pad flag of the attention kernels is one per batch).  The price is workspace: the fp32 score maps take
 * S(1)*B*H*C*Cp*4 bytes, where esmk_msa_forward takes S(B) of them — up to 8 x its buffer at a large B on a small MSA (S(1) <= 8,
 * S(B) falls to 1 once B*H*ceil(C/256)^2 tiles fill the GPU); ask esmk_msa_rows_workspace_bytes, not esmk_msa_workspace_bytes.
 * vocab <= 64, MSA handles only (esmk_forward_rows serves the single-sequence models), the shape limits of
 * esmk_msa_forward.  The whole call runs on `stream`; error messages name esmk_msa_forward_rows. */
int esmk_msa_rows_workspace_bytes(const esmk_model* m, int B, int R, int C, int n_sel, size_t* bytes, size_t* logits_offset);
int esmk_msa_forward_rows(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int R, int C,
                          const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
/* The number of K slices the workspace plan of an MSA forward takes for the tied-row score GEMM (no GPU needed):
 * rows_entry 0 = esmk_msa_forward at this B, 1 = esmk_msa_forward_rows (the count of B = 1, whatever B is). */
int esmk_debug_msa_row_slices(const esmk_model* m, int B, int R, int C, int rows_entry, int32_t* slices);

/* Per-kernel-class timing of esmk_forward with HIP events recorded on the launch stream
 * (measurement support for bench.py; the reference has no counterpart).
 * esmk_profile_begin() arms it; every launch of the following esmk_forward() calls is bracketed
 * by two events; esmk_profile_end() waits for them and returns one aggregated entry per class:
 * launches, total milliseconds, algorithmic FLOPs and algorithmic bytes. */
typedef struct esmk_profile_entry {
    char name[32];
    int32_t launches;
    double ms;
    double flops;
    double bytes;
} esmk_profile_entry;
int esmk_profile_begin(esmk_model* m);
int esmk_profile_end(esmk_model* m, esmk_profile_entry* out, int max_entries, int* n_out);
/* 1 if the handle runs with the LayerNorm fold (esmk_config::ln_fold resolved against the library default and
 * ESMK_LN_FOLD), 0 if not, -1 for a null / MSA handle.  Measurement scripts record the mode next to their numbers. */
int esmk_ln_fold_enabled(const esmk_model* m);

/* ---- single-kernel entry points (used by the parity tests and micro-benchmarks) -------- */

/* ESM1bLayerNorm == torch.nn.LayerNorm(E, eps=1e-5) (esm/modules.py:68-81).
 * x fp32 [rows,E] -> y (operand dtype) [rows,E] and/or y32 fp32 [rows,E] (either may be NULL).
 * Bits 8..11 of operand_dtype select the kernel form for tests: 0 = default (the engine's form), else variant + 1 with
 * variant 0 = the plain one-row-per-wave form and 7 = the engine's form by name; any other variant is an error. */
int esmk_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev,
                      void* y_dev, float* y32_dev, int rows, int E, int operand_dtype,
                      void* stream);

/* Mean representation of every sequence of a batch, as scripts/extract.py:113-116 computes it on the host
 * (`t[i, 1 : truncate_len + 1].mean(0)`): out[b,:] (fp32 [B,E]) = mean of rows [first_row, first_row + n_b) of
 * x[b] ([B,T,E] in dtype code x_dtype), n_b = min(count_dev[b], T - first_row); an empty slice yields NaN like
 * torch.mean.  One pass over x, deterministic (no atomics). */
int esmk_op_masked_row_mean(const void* x_dev, int x_dtype, const int32_t* count_dev, float* out_dev, int B, int T,
                            int E, int first_row, void* stream);

/* nn.Linear: C[M,N] = A[M,K] . W[N,K]^T + bias, epilogue selected by `epilogue`:
 *   0 plain -> out operand dtype [M,N]           1 plain -> out fp32 [M,N]
 *   2 gelu (modules.py:17-24) -> operand dtype   3 gelu -> fp32
 *   4 residual: out fp32 [M,N] += result         (modules.py:134,140)
 * A, W operand dtype; bias fp32 (may be NULL).  Bits 12..19 of operand_dtype must be 0. */
int esmk_op_linear(const void* a_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                   int M, int N, int K, int epilogue, int operand_dtype, void* stream);

/* Measurement hook (no reference counterpart; tools/bench_splitk.py): S fp32 partial products
 * out[s][M,N] = A[:, sK/S:(s+1)K/S] . W[:, sK/S:(s+1)K/S]^T as ONE batched launch of the persistent kernel
 * (K/S a multiple of 64).  Small-batch study: a [4096,5120]x[1280,5120] GEMM has 80 tiles for 256 CUs. */
int esmk_debug_linear_splitk(const void* a_dev, const void* w_dev, float* partials_dev, int M, int N, int K,
                             int S, int operand_dtype, void* stream);

/* Measurement hook (no reference counterpart): when stamps_dev != NULL every following persistent
 * GEMM launch records s_memtime stamps per workgroup and tile, uint64 [256][32][4] =
 * {tile start, main loop done, epilogue done, unused}; NULL switches it off. */
int esmk_debug_gemm_timing(void* stamps_dev);

/* Split-weight GEMM of the f16x2 precision mode as single ops (tests, tools/bench_gemm9.py):
 * esmk_op_split_weight: w [N,K] (any float dtype) -> w2 fp16 [N,2K], K tiles of 64 columns interleaved hi | lo with
 * hi = fp16(w), lo = fp16(w - hi);  esmk_op_linear_split: out = a[M,K] . (w_hi + w_lo)^T + bias with the epilogues of
 * esmk_op_linear (K % 64 == 0, N % 8 == 0). */
int esmk_op_split_weight(const void* w_dev, int w_dtype, void* w2_dev, int N, int K, void* stream);
int esmk_op_linear_split(const void* a_dev, const void* w2_dev, const float* bias_dev, void* out_dev, int M, int N, int K,
                         int epilogue, void* stream);

/* The kernels the precision modes (esmk_config::weight_split) are built from, one launch at a time (tests).  Each entry makes
 * exactly the launch the engine makes and refuses, before any HIP call, what the kernel's address arithmetic does not cover;
 * the extent of the buffers is the caller's.
 * esmk_op_linear_f32: the exact-fp32 MFMA linear of the LM head (gemm32.hip): out[M,N] (row stride ldc) = act(a[M,K] (row
 *   stride lda) . w[N,K]^T + bias), act = gelu (modules.py:17-24) when gelu != 0; all fp32, bias may be NULL.
 *   K % 32 == 0, lda % 4 == 0, lda >= K, ldc >= N.
 * esmk_op_layernorm_ex: esmk_op_layernorm with every field of the engine's LayerNorm launch: row_keep fp32 [rows] (output
 *   rows multiplied by it, msa_transformer.py:171-172) or NULL; map_R > 0: input row (b,r,c) of [B,map_R,map_C] is written to
 *   output row (b,c,r), rows % (map_R map_C) == 0; ldy = row stride of y in elements (0 = E, else >= E and a multiple of 4; y32
 *   rows always have stride E); x3 != 0: y rows in the f16x3 operand layout, per 64-column K tile hi | hi | lo with hi = fp16(o),
 *   lo = fp16(o - hi) (fp16 only, E % 64 == 0, ldy >= 3 E, y required); eps > 0 (1e-5; 1e-12 for ESM-1).  E % 4 == 0,
 *   E <= 5120.  operand_dtype carries the kernel variant as in esmk_op_layernorm (bits 8..11 = variant + 1; default, 0 or 7).
 * esmk_op_split_weight_ex: the weight images: w [rows,cols] (any float dtype) -> parts = 1: dst [.., dst_ld] in dst_dtype, a
 *   plain conversion; parts = 2 / 3: dst fp16 [.., parts dst_ld], 64-column K tile t of a row as hi | lo (f16x2) or
 *   hi | lo | hi (f16x3) at columns 64 parts t, dst_ld % 64 == 0.  row_map / col_map = 1 spread heads of head_dim d over 64
 *   slots: index h d + i -> 64 h + (i < d / 2 ? i : 32 + i - d / 2) (d in 1..64; slots in between are NOT written); d = 128:
 *   128 h + the dims in the order [0,32) | [64,96) | [32,64) | [96,128).  d must divide the mapped extent; dst_ld >= the
 *   mapped column extent.
 * esmk_op_linear_gelu_x3: fc1 + GELU of the f16x3 mode (gemm9.hip): a3 fp16 [M,K3] rows hi | hi | lo, w3 fp16 [N,K3] rows
 *   hi | lo | hi, bias fp32 [N] -> out3 fp16 [M,3N], gelu(a . w^T + bias) as hi | hi | lo per 64 columns.  K3 % 192 == 0,
 *   N % 64 == 0 (the hi | hi | lo store of a 64-column block would leave a shorter row). */
int esmk_op_linear_f32(const float* a_dev, int lda, const float* w_dev, const float* bias_dev, float* out_dev, int ldc, int M,
                       int N, int K, int gelu, void* stream);
int esmk_op_layernorm_ex(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, float* y32_dev,
                         int rows, int E, int operand_dtype, const float* row_keep_dev, int map_R, int map_C, int ldy, int x3,
                         float eps, void* stream);
int esmk_op_split_weight_ex(const void* w_dev, int w_dtype, void* dst_dev, int dst_dtype, int rows, int cols, int dst_ld,
                            int parts, int row_map, int col_map, int head_dim, void* stream);
int esmk_op_linear_gelu_x3(const void* a3_dev, const void* w3_dev, const float* bias_dev, void* out3_dev, int M, int N, int K3,
                           void* stream);

/* Toolchain guard (no reference counterpart): the attention / contact kernels issue one MFMA per key tile through inline
 * asm (its C operand, the softmax offset broadcast, must survive); the compiler does not see that instruction's hazards.
 * Runs it beside the builtin on the same operands: a, b [64][8] operand dtype, c [64][16] fp32, out [3][64][16] fp32 =
 * {asm path, builtin path, c after the calls}; the first two must be bit-equal, the third equal to 2 c
 * (tests/test_kernels_gpu.py runs it on every GPU test run, i.e. on every toolchain the library is built with). */
int esmk_debug_mma_selftest(const void* a_dev, const void* b_dev, const float* c_dev, float* out_dev, int operand_dtype,
                            void* stream);

/* Measurement / A-B hook (no reference counterpart): which persistent GEMM kernel serves the dense nn.Linear calls
 * from now on — 8 = gemm8.hip (two waves per SIMD), 9 = gemm9.hip (one wave per SIMD, 128 x 128 wave blocks;
 * bit-identical results) wherever it applies, 0 = the library's own choice per call (default).  `variant` must be 0:
 * gemm9 has one form (the issue patterns and timing experiments the argument once selected are in the project's git
 * history and profiles/).  The environment variable ESMK_GEMM_IMPL=8|9|auto sets the same thing for a
 * whole process. */
int esmk_debug_gemm_impl(int impl, int variant);

/* What the library would launch for a dense nn.Linear call (no reference counterpart, no GPU needed): out =
 * {kernel, half_m, 0, 0}; kernel 9 = gemm9.hip, 8 = gemm8.hip, 256 / 64 = the one-tile-per-workgroup kernels of
 * gemm.hip, 0 = no kernel takes the call; half_m 1 = 128-row tiles.  epilogue: the codes of esmk_op_linear, 5 / 6 = the
 * q, k / v projections, 7 = the MSA row-attention context, 8 = q, k and v in one launch (N = 3E).  flags: 1 = the
 * force_generic and 2 = the force_old test hook of esmk_op_linear, 4 = the LayerNorm-fold form of the epilogue (producer
 * for 4, consumer for 2, 5, 6, 8; an error for the others), 8 = the split-weight form of esmk_op_linear_split (K as
 * there), 16 = a batched call (generalised addressing, batch = 2), 32 = the f16x3 output form of esmk_op_linear_gelu_x3 (epilogue
 * 2 and no other flag; an error otherwise): kernel 9, or 0 where N % 64 != 0.  Follows ESMK_GEMM_IMPL / esmk_debug_gemm_impl. */
int esmk_debug_gemm_plan(int M, int N, int K, int epilogue, int flags, int32_t out[4]);

/* Measurement / A-B hook (no reference counterpart): named switches of the library, process wide.  No switch changes a
 * result bit.  "qkv_one_launch": 1 / 0 = always / never run the q, k and v projections of a layer as ONE GEMM launch,
 * -1 = the library's choice (one launch where it needs fewer rounds of tiles over the CUs, i.e. small batches;
 * gemm_dispatch.hip; environment: ESMK_QKV_ONE_LAUNCH).  The one exception to "no result bit" is "rows_contacts_own_groups":
 * 1 makes esmk_forward_rows_contacts (and its workspace query) take the head-group count of the batch instead of the pinned
 * one of B = 1, so that what the pin costs can be timed (tools/design_throughput.py); the maps then carry the bits of
 * esmk_forward at that B.  0, the default, is the pin.  Any other key is an error ("unknown key"). */
int esmk_debug_set(const char* key, double value);

/* Fused q/k/v projection + scaling + rotary + head split (multihead_attention.py:256-284,
 * :354-355; rotary_embedding.py:11-20).  a [B*T,E]; wqkv [3E,E]; bias [3E];
 * q_out,k_out [B,H,T,64]; vt_out [B,H,64,Tp] (V transposed, keys permuted in groups of 16,
 * Tp = T rounded up to 64; see attention.hip). */
int esmk_op_qkv_rope(esmk_model* m, const void* a_dev, const void* wqkv_dev,
                     const float* bias_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                     void* stream);
/* The same with the score domain made explicit: log2_domain = 1 folds log2(e) into the q scale as well (one rounding
 * to the operand dtype), which is the q esmk_op_attention / esmk_op_attention_probs expect — the two ops then compose
 * without a conversion; log2_domain = 0 is esmk_op_qkv_rope (q scaled by d^-1/2 only, the reference's q). */
int esmk_op_qkv_rope2(esmk_model* m, const void* a_dev, const void* wqkv_dev,
                      const float* bias_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                      int log2_domain, void* stream);

/* LayerNorm fold (esmk_config::ln_fold) as single ops — the pieces esmk_forward chains per layer (modules.py:120-140):
 * esmk_op_rowstats: x fp32 [rows,E] -> y[row][c] = T(x - mean) (row stride ldy, operand dtype), mean[row], rstd[row]
 *   (eps 1e-5, biased variance: the statistics of ESM1bLayerNorm, modules.py:68-81);
 * esmk_op_fold_weight: w [N,K] of the Linear that follows a LayerNorm(gamma, beta) -> dst[n][k] = T(w[n][k] gamma[k] -
 *   mean_k(w[n][.] gamma[.])) (row stride ld), bias2[n] = sum_k w[n][k] beta[k];
 * esmk_op_linear_ln, epilogue 2 (consumer): out = T(gelu(ln_rstd[m] * (a . w^T) + bias + bias2)), a = the rows of
 *   rowstats / of a producer, w = a folded image;  epilogue 4 (producer): out fp32 [M,N] += a . w^T + bias, and
 *   h16[m][n] = T(out_new - ln_mean[m]) (row stride ldh), ln_part[m][n / 128] = (sum, sum of squares) of out_new -
 *   ln_mean[m] over the 128 columns (ln_parts >= ceil(N / 128) entries per row);
 * esmk_op_ln_finalize: ln_part -> mean[row] += sum / E, rstd[row] = rsqrt(var + 1e-5);
 * esmk_op_qkv_rope_ln: esmk_op_qkv_rope2 with folded wqkv and the rows' rstd (ln_rstd must be readable up to the next
 *   multiple of 256 rows). */
int esmk_op_rowstats(const float* x_dev, void* y_dev, float* mean_dev, float* rstd_dev, int rows, int E, int ldy,
                     int operand_dtype, void* stream);
int esmk_op_ln_finalize(const float* part_dev, float* mean_dev, float* rstd_dev, int rows, int parts, int E, void* stream);
int esmk_op_fold_weight(const void* w_dev, int w_dtype, const float* gamma_dev, const float* beta_dev, void* dst_dev,
                        int dst_dtype, float* bias2_dev, int N, int K, int ld, void* stream);
/* esmk_op_fold_weight with the head spread of models whose head_dim is below 64 (q / k / v rows): head_dim 16 / 24 / 32:
 * row head * d + i of w goes to row head * 64 + (i < d / 2 ? i : 32 + i - d / 2) of dst and bias2 (N / d * 64 rows; the rows
 * in between are left as they are); head_dim 64: the identity.  N must hold whole heads. */
int esmk_op_fold_weight_ex(const void* w_dev, int w_dtype, const float* gamma_dev, const float* beta_dev, void* dst_dev,
                           int dst_dtype, float* bias2_dev, int N, int K, int ld, int head_dim, void* stream);
int esmk_op_linear_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const float* bias2_dev, void* out_dev,
                      int M, int N, int K, int epilogue, int operand_dtype, const float* ln_rstd_dev, void* h16_dev, int ldh,
                      float* ln_part_dev, int ln_parts, const float* ln_mean_dev, int half_m, void* stream);
int esmk_op_qkv_rope_ln(esmk_model* m, const void* a_dev, const void* wqkv_dev, const float* bias_dev,
                        const float* bias2_dev, const float* ln_rstd_dev, void* q_out, void* k_out, void* vt_out, int B, int T,
                        int log2_domain, void* stream);

/* softmax(q k^T + key_bias) v  (multihead_attention.py:357-394), flash style.
 * SCORE DOMAIN: q must carry log2(e) besides d^-1/2 (esmk_forward's QKV epilogue folds both into the q scale
 * before the single rounding to the operand dtype); q.k is then the score in the log2 domain, the kernel's
 * exponentials are exp2, and lse_out is the row log2-sum-exp2 (= natural lse * log2 e).
 * esmk_op_attention_probs takes the same q and that lse.  (esmk_op_qkv_rope scales q by d^-1/2 only.)
 * key_bias fp32 [B,T] (0 or -inf, NULL = no padding); ctx_out [B*T, H*64] operand dtype;
 * lse_out fp32 [B,H,T] or NULL. */
int esmk_op_attention(const void* q_dev, const void* k_dev, const void* vt_dev,
                      const float* key_bias_dev, void* ctx_out, float* lse_out, int B, int H,
                      int T, int operand_dtype, void* stream);

/* Per-head attention probabilities (multihead_attention.py:396-403, esm2.py:132-139):
 * probs_out fp32 [B, Ltot, H, T, T] slice `layer`, rows/cols of padded tokens zeroed. */
int esmk_op_attention_probs(const void* q_dev, const void* k_dev, const float* lse_dev,
                            const float* key_bias_dev, float* probs_out, int B, int H, int T,
                            int layer, int num_layers_total, int operand_dtype, void* stream);

/* Every form of the attention core the engine launches, one kernel at a time (tests / micro-benchmarks; no reference
 * counterpart beyond the two entries above).  Same score domain as esmk_op_attention; vt [B,H,head_dim,Tp], Tp a
 * multiple of 64 and >= T.
 *   mode 0: key_bias fp32 [B,T] (0 / -inf, or NULL); seq_info int32 [B,2] = (#pads, 1 + index of the last non-pad
 *           token) as esmk_forward computes it, or NULL (needs key_bias); head_dim 64 or 128.  With seq_info, all-pad
 *           key tiles behind the last real token are skipped and padded query rows give finite values (ctx and lse
 *           0 for a sequence of padding only).  ctx_out [B*T, H*head_dim].
 *   mode 1: MSA column attention (axial_attention.py:207-218): key_bias holds 0/1 fill flags, used only when the
 *           device int *any_pad_dev != 0 (NULL = 0); a flagged key's score is REPLACED by -10000; head_dim 64.
 *   mode 2: precision mode f16x3: ctx_out [B*T, 3*H*64], per head hi | hi | lo with lo = fp16(v - hi); head_dim 64,
 *           fp16 only.
 * lse_out fp32 [B,H,T] (log2 domain) or NULL.  Invalid combinations fail before the HIP runtime is touched. */
int esmk_op_attention_ex(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                         const int32_t* seq_info_dev, const int32_t* any_pad_dev, void* ctx_out, float* lse_out, int B,
                         int H, int T, int Tp, int head_dim, int mode, int operand_dtype, void* stream);
/* esmk_op_attention_ex mode 0 (head_dim 64, padded batch) with the learned null key / value pair of the ESM-1 models:
 * bias_k_dev / bias_v_dev [H,64] in the operand dtype, bias_k in k's domain (unscaled: q carries d^-1/2 log2 e).  Every query
 * row sees T + 1 keys, the extra one never masked; ctx_out and lse_out include it, so esmk_op_attention_probs* on the same
 * q / k / lse give the maps with the null column dropped. */
int esmk_op_attention_biaskv(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                             const int32_t* seq_info_dev, const void* bias_k_dev, const void* bias_v_dev, void* ctx_out,
                             float* lse_out, int B, int H, int T, int Tp, int operand_dtype, void* stream);
/* Probabilities of every form: msa_C = 0 is the ESM-2 layout probs_out [B, Ltot, H, T, T] (rows / cols of padded
 * tokens zeroed, head_dim 64 or 128, out_dtype fp32 or the operand dtype); msa_C > 0 is the MSA column layout
 * [B / msa_C, Ltot, H, msa_C, T, T] (B = batch x columns, key_bias = fill flags with any_pad_dev as in mode 1, query rows
 * not zeroed, head_dim 64, fp32). */
int esmk_op_attention_probs_ex(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                               const int32_t* any_pad_dev, void* probs_out, int B, int H, int T, int head_dim, int layer,
                               int num_layers_total, int msa_C, int out_dtype, int operand_dtype, void* stream);

/* The attention core of a token-packed batch, one kernel at a time (multihead_attention.py:357-394 per segment; tests /
 * micro-benchmarks).  q, k [H,rows,head_dim] and vt [H,head_dim,Tp] in the layouts and the score domain of
 * esmk_op_attention_ex (B = 1, T = rows), Tp a multiple of 64 and >= rows + 64: the last key tile of a segment may reach
 * 63 columns past the last row, and the columns of vt behind the segments' rows must be finite (zero).
 * segments_host int32 [n_seg][2] = (first row, length): starts are ascending multiples of 16, segments disjoint, gaps
 * allowed anywhere (also in front of the first segment); rows % 64 == 0.  key_bias fp32 [rows] (0 / -inf) or NULL; the
 * per-segment <pad> counts the kernel wants are derived from it on the device.  ctx_out [rows, H*head_dim] operand dtype,
 * rows outside every segment are not written; lse_out fp32 [H,rows] (log2 domain) or NULL.  Every segment's rows carry
 * the bits esmk_op_attention_ex (mode 0) gives that segment alone — with seq_info when its <pad> tokens are interior,
 * without when they trail (the engine never packs trailing pads: a segment ends at its last real token).  A segment of
 * padding only has no key to attend to: its ctx and lse rows are cleared to 0 by a second small launch, the values the
 * padded form gives such a sequence through seq_info.  That clearing step belongs to THIS entry only: esmk_forward_packed*
 * do not launch it, so there the context row of an all-<pad> sequence (a one-row segment) is 1 / 0 = NaN, confined to that
 * row — its attention map is still exactly zero (the query-row select), and no other row reads it.  head_dim 64 or 128.
 * bias_k_dev / bias_v_dev must be NULL and are refused otherwise (the null key of the ESM-1 models has no packed form;
 * the slot keeps the signature stable).  The entry uploads a small work list of its own, waits for the stream and
 * frees it: it owns no persistent state.  Invalid arguments fail before the HIP runtime is touched. */
int esmk_op_attention_packed(const void* q_dev, const void* k_dev, const void* vt_dev, const float* key_bias_dev,
                             const int32_t* segments_host, int n_seg, int rows, int Tp, int H, int head_dim,
                             int operand_dtype, const void* bias_k_dev, const void* bias_v_dev, void* ctx_out, float* lse_out,
                             void* stream);
/* The attention maps of a token-packed batch, one kernel at a time (multihead_attention.py:396-403 per segment, slice
 * `layer` of the stack esm2.py:132-139 builds): q, k, key_bias and the segment table as above, lse fp32 [H,rows] from
 * esmk_op_attention_packed.  probs_out is the ragged buffer of esmk_forward_packed_maps with L = L_total (segment s's
 * [L_total,H,len_s,len_s] block at L_total * H * sum_{s'<s} len_s'^2), fp32 or, with lowp != 0, the operand dtype;
 * probs_elems is checked against L_total * H * sum(len^2) before any launch.  Each map carries the bits
 * esmk_op_attention_probs_ex gives that segment alone.  Same ownership rule as above. */
int esmk_op_attention_probs_packed(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                                   const int32_t* segments_host, int n_seg, int rows, int H, int head_dim, int L_total,
                                   int layer, int operand_dtype, int lowp, void* probs_out, size_t probs_elems, void* stream);

/* The fused contact pipeline of predict_contacts (contacts.hip: accumulate + reduce per layer, then rt + final) on
 * caller-supplied operands, one entry for the padded and the token-packed form.  Inputs are stacked over layers in the
 * layouts esmk_forward leaves in its workspace:
 *   padded (segments_host NULL, n_seg 0): q, k [L, B, H, T, head_dim] (q in the log2 domain, as esmk_op_attention takes
 *     it), lse fp32 [L, B, H, T] (log2 domain), key_bias fp32 [B, T] (0 / -inf) or NULL, tokens int64 [B, T];
 *     out fp32 [B, S, S], S = T - prepend_bos - append_eos > 0.
 *   packed (segments_host = int32 [n_seg][2] (first row, length), B = 1, T = rows): q, k [L, H, rows, head_dim], lse
 *     [L, H, rows], key_bias [rows] or NULL, tokens [rows]; out is the ragged buffer of esmk_forward_packed_ex (each
 *     segment with S_s > 0 in table order, [S_s, S_s] at sum of the previous S^2).  Segments may leave gaps, start at
 *     any row, come in any order and be empty; they must not overlap.
 * w fp32 [L*H] (contact_head.regression.weight), b fp32 [1] or NULL.  head_groups: 0 = the engine's head-group count,
 * else 1 <= G <= H (head_dim 128: at most 20 heads per group), raised to ceil(H / ceil(H / G)) so that every group holds
 * a head; *head_groups_used (optional) receives the count that ran.  Invalid arguments fail before any launch. */
int esmk_op_contacts_fused_workspace_bytes_ex(int B, int H, int T, int num_layers, int head_dim,
                                              const int32_t* segments_host, int n_seg, int prepend_bos, int append_eos,
                                              int head_groups, size_t* bytes);
int esmk_op_contacts_fused_ex(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                              const int64_t* tokens_dev, const float* w_dev, const float* b_dev,
                              const int32_t* segments_host, int n_seg, float* out_dev, void* workspace_dev,
                              size_t workspace_bytes, int B, int H, int T, int num_layers, int head_dim, int pad_idx,
                              int eos_idx, int prepend_bos, int append_eos, int head_groups, int* head_groups_used,
                              int operand_dtype, void* stream);

/* The generalised-addressing GEMM forms the engine launches (MSA Transformer, head_dim 128, token-packed rotary
 * positions), one launch at a time (tests).  One field per field of the engine's internal GemmArgs, with the same
 * meaning (esm_amd/csrc/kernels.h); 0 / NULL = the dense default.  `size` = sizeof(esmk_gemm_ex_args).  Operand rows
 * and byte offsets are the caller's: the entry checks the shape rules below, not the extent of the buffers.
 *   out = A . W^T + bias through `epilogue` (0 store, 1 fp32 store, 2 gelu, 4 fp32 residual add, 5 q/k + rotary,
 *   6 v transposed, 7 MSA row-attention context); batched: entry z = zo * batch_inner + zi reads A + zo a_bo + zi a_bi,
 *   W + zo w_bo + zi w_bi and writes out + zo o_bo + zi o_bi (bytes).
 * Refused before any HIP call: null operands or outputs, K % 64 != 0, N % 8 != 0, N % 64 != 0 for epilogues 5, 6
 * and 7, head_dim not 64 / 128, batch_inner not dividing batch, vt_rows with head_dim 128, epilogue 3 (fp32 gelu)
 * with any generalised field.  The LayerNorm-fold and f16x3 forms have entries of their own and no field here. */
typedef struct esmk_gemm_ex_args {
    size_t size;
    const void* A;
    const void* W;
    const float* bias;
    void* out;
    int32_t M, N, K;
    int32_t a_kt_repeat;
    int64_t a_row_bytes, w_row_bytes, a_kt_bytes, w_kt_bytes;
    int32_t batch, batch_inner;
    int64_t a_bo, a_bi, w_bo, w_bi, o_bo, o_bi;
    int32_t n_valid, ldc;
    void* q;
    void* k;
    void* vt;
    const float* cos;
    const float* sin;
    int32_t T, H, E, Tp;
    float scaling;
    int32_t vt_rows;
    const float* row_keep;
    int32_t rowmap_R, rowmap_C, ctx_R, ctx_C;
    int32_t head_dim;
    int32_t epilogue;
    const int32_t* row_pos;
    int32_t operand_dtype;
    int32_t reserved;
} esmk_gemm_ex_args;
int esmk_op_gemm_ex(const esmk_gemm_ex_args* args, void* stream);

/* Tied row-attention softmax of the MSA Transformer (axial_attention.py:96-100,127): scores fp32 [B, nslice, H, C, ldp]
 * (nslice partial maps, summed in index order), keep fp32 [B, R, C] (1 - pad; columns padded in MSA row 0 get -10000
 * when the device int *any_pad != 0), probs_out operand dtype [B, H, C, ldp] with columns [C, ldp) set to 0, attn_out
 * fp32 [B, num_layers_total, H, C, C] slice `layer`, or NULL.  C <= ldp <= 1024, nslice >= 1. */
int esmk_op_msa_row_softmax(const float* scores_dev, const float* keep_dev, const int32_t* any_pad_dev, void* probs_out,
                            float* attn_out, int B, int H, int R, int C, int ldp, int layer, int num_layers_total,
                            int nslice, int operand_dtype, void* stream);

/* The kernels of esmk_forward_rows' callers, one launch at a time (tests).
 * esmk_op_mask_rows: the masked batch of the masked-marginal strategy (predict.py:208-209 for n positions at once):
 *   out int64 [n,T], row i = tokens[src_row[i], :] (tokens int64 [B,T]; src_row int32 [n] or NULL = row 0, clamped to
 *   [0,B)) with position pos[i] (int32 [n]) replaced by mask_idx; a position outside [0,T) masks nothing.
 * esmk_op_log_softmax_rows: out fp32 [n,V] = log_softmax(logits fp32 [n,V]) = x - max - log(sum exp(x - max)), V <= 64;
 *   target int32 [n] (with target_out fp32 [n], both or neither): target_out[i] = out[i, clamp(target[i], 0, V-1)]. */
int esmk_op_mask_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_dev, int64_t* out_dev, int B,
                      int T, int n, int mask_idx, void* stream);
int esmk_op_log_softmax_rows(const float* logits_dev, float* out_dev, const int32_t* target_dev, float* target_out_dev, int n,
                             int V, void* stream);

/* Multi-mutant variants (the ESM-1v paper's masked-marginal score of a variant with several substitutions: mask ALL of its
 * positions at once, one forward, sum log p(mt) - log p(wt) over them).
 * esmk_op_mask_rows_multi: out int64 [n,T], row i = tokens[src_row[i], :] (as esmk_op_mask_rows) with every position of
 *   pos[pos_off[i] : pos_off[i+1]] replaced by mask_idx; pos_off int32 [n+1], pos int32 [total].  All lists are device
 *   data: a source row outside [0,B) is clamped, the offsets are clamped to [0,total], a pair with hi < lo is an empty
 *   list (a plain copy), a position outside [0,T) masks nothing, a repeated position is harmless.
 * esmk_op_score_rows: out fp64 [n_var], out[v] = sum over r in [var_off[v], var_off[v+1]), r ascending, of
 *   (logprobs[r, mt[r]] - logprobs[r, wt[r]]); logprobs fp32 [n_rows,V], wt / mt int32 [n_rows], var_off int32 [n_var+1].
 *   Each term is the fp32 difference; the terms are added in fp64 in index order by one lane per variant (no atomics), so
 *   the result does not depend on the launch geometry.  Columns are clamped to [0,V), offsets to [0,n_rows]; an empty
 *   range gives 0.0.
 * Refused before any HIP call: null pointers (src_row_dev may be NULL), B, T, n, n_rows, n_var or V <= 0, total < 0. */
int esmk_op_mask_rows_multi(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_off_dev,
                            const int32_t* pos_dev, int64_t* out_dev, int B, int T, int n, int total, int mask_idx, void* stream);
int esmk_op_score_rows(const float* logprobs_dev, const int32_t* wt_dev, const int32_t* mt_dev, const int32_t* var_off_dev,
                       double* out_dev, int n_rows, int n_var, int V, void* stream);

/* Mixed-length libraries scored token-packed (esmk_forward_packed_rows).
 * esmk_op_mask_rows_packed: the packed counterpart of esmk_op_mask_rows_multi.  out int64 [rows] is ONE packed row space; copy i
 *   is the first seg_len[i] tokens of tokens[src_row[i], :] (tokens int64 [B,T]) written to out[seg_start[i] : seg_start[i] +
 *   seg_len[i]] with every position of pos[pos_off[i] : pos_off[i+1]] replaced by mask_idx, and the gap behind the copy — up to
 *   seg_start[i+1], or to `rows` behind the last copy — filled with pad_idx: every row from seg_start[0] on is written, nothing
 *   is assumed about what out held (esmk_forward_packed wants pad_idx in gap rows).  src_row, seg_start, seg_len int32 [n],
 *   pos_off int32 [n+1], pos int32 [total], all on the device and never read by the host: a source row outside [0,B) is
 *   clamped, seg_start to [0,rows], seg_len to [0,T] and to the rows left behind seg_start (nothing is written outside
 *   [0,rows)), the offsets to [0,total], a pair with hi < lo is an empty list, a position outside [0,seg_len) masks nothing,
 *   a repeated position is harmless.  The copies' row ranges must be ascending and disjoint.
 * esmk_op_sum_target_rows: out fp64 [n_seq], out[s] = sum over r in [off[s], off[s+1]), r ascending, of logprobs[r, target[r]];
 *   logprobs fp32 [n_rows,V], target int32 [n_rows], off int32 [n_seq+1].  fp32 terms added in fp64 in index order by one lane
 *   per sequence (no atomics).  target is clamped to [0,V), offsets to [0,n_rows]; an empty range gives 0.0.
 * Refused before any HIP call: null pointers, B, T, n, n_rows, n_seq or V <= 0, total < 0, rows <= 0, rows % 64 != 0,
 * rows > 2^24, B*T > 2^24. */
int esmk_op_mask_rows_packed(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* seg_start_dev,
                             const int32_t* seg_len_dev, const int32_t* pos_off_dev, const int32_t* pos_dev, int64_t* out_dev, int B,
                             int T, int n, int total, int rows, int mask_idx, int pad_idx, void* stream);
int esmk_op_sum_target_rows(const float* logprobs_dev, const int32_t* target_dev, const int32_t* off_dev, double* out_dev,
                            int n_rows, int n_seq, int V, void* stream);

/* Proteins longer than the model's window (esm_amd/windows.py): window copies built on the device, per-window outputs stitched
 * into full-length outputs.  A window of Tw tokens starting at source token s covers the source tokens s .. s + R - 1; wrapped
 * (a fragment tokenised as the alphabet tokenises the substring) it carries <cls> in column 0 and / or <eos> in column Tw - 1
 * and R = Tw minus those; raw it is a token slice, R = Tw.
 * esmk_op_window_rows: out int64 [n,Tw]; copy i, column c = tokens[clamp(src_row[i]), clamp(start[i] + c - h)] (tokens int64
 *   [B,T]; src_row, start int32 [n]; h = 1 if head_tok >= 0 else 0; the row is clamped to [0,B), the column to [0,T)); column
 *   0 is head_tok when head_tok >= 0 and column Tw - 1 is tail_tok when tail_tok >= 0.  mask_off int32 [n+1], mask_pos int32
 *   [total]: the entries mask_pos[mask_off[i] : mask_off[i+1]] are token coordinates of the SOURCE row; entry p becomes mask_idx at
 *   column p - start[i] + h where that is a body column of the copy (h <= column < Tw - (tail_tok >= 0)); an entry outside the
 *   copy's range or on an overridden column masks nothing, a repeated entry is harmless.  The offsets are clamped to [0,total],
 *   a pair with hi < lo is an empty list, as in esmk_op_mask_rows_multi.
 * esmk_op_blend_rows: out fp32 [n_out,E], out[r] = (sum_k w[k] x[src[k], :]) / sum_k w[k] over k in [off[r], off[r+1]), k
 *   ascending; x [N,E] of dtype code x_dtype (ESMK_F32 / ESMK_F16 / ESMK_BF16, as esmk_op_masked_row_mean), off int32 [n_out+1],
 *   src int32 [total], w fp32 [total] (positive).  Every element is accumulated in fp32 in list order by one lane (no atomics):
 *   the result does not depend on the launch geometry.  A list of ONE entry copies the row, converted to fp32, exactly (the
 *   owner stitch: w is not read); an empty list gives zeros.  src is clamped to [0,N), the offsets to [0,total].
 * esmk_op_stitch_contacts: out fp32 [Lb,Lb]; maps fp32 [n_w,R,R], window w covering the residues s_w .. s_w + R - 1 with
 *   s_w = start[w] - body_lo (start int32 [n_w], device data).  out[i,j] = maps[w, i - s_w, j - s_w] of the window that holds both
 *   residues with the least |2 s_w + R - 1 - (i + j)| (integers), a tie going to the lower start; NaN where no window holds both.
 * Refused before any HIP call: null pointers, B, T, n, Tw, N, n_out, n_w, R or Lb <= 0, total < 0, E <= 0 or E % 4 != 0, an
 * unknown x_dtype, B*T or n*Tw > 2^24. */
int esmk_op_window_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* start_dev,
                        const int32_t* mask_off_dev, const int32_t* mask_pos_dev, int64_t* out_dev, int B, int T, int n, int Tw,
                        int total, int head_tok, int tail_tok, int mask_idx, void* stream);
int esmk_op_blend_rows(const void* x_dev, int x_dtype, const int32_t* off_dev, const int32_t* src_dev, const float* w_dev,
                       float* out_dev, int N, int E, int n_out, int total, void* stream);
int esmk_op_stitch_contacts(const float* maps_dev, const int32_t* start_dev, float* out_dev, int n_w, int R, int Lb, int body_lo,
                            void* stream);

/* Drawing sequences from the model (esm_amd/sampling.py: Gibbs sweeps, mask in-painting).  A sampling step is
 * esmk_op_mask_rows_multi -> esmk_forward_rows -> esmk_op_sample_rows -> esmk_op_commit_tokens on one stream; the host reads
 * nothing in between.  Confidence-ordered unmasking is esmk_forward_rows on every remaining <mask> row -> esmk_op_sample_rows_ex
 * (a draw and a score per row) -> esmk_op_select_rows (the best rows of every chain) -> esmk_op_commit_tokens.  Random numbers are plain Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key bumps 0x9E3779B9 /
 * 0xBB67AE85, ten rounds) with key = (seed & 0xffffffff, seed >> 32) and counter = (chain id, epoch or step, purpose, index),
 * purpose 0 = permutation, 1 = token draw.  A number depends on these words alone — never on a thread or block index, the
 * batch size or the launch geometry — so a chain draws the same tokens alone and inside any batch.  A uniform is
 * u = (word0 >> 8) * 2^-24: exact in fp32, in [0,1).  No atomics; all list data is device data the host never reads.
 * esmk_op_permute_positions: per chain c the slice [pos_off[c], pos_off[c+1]) of perm_out int32 [total] is a Fisher-Yates
 *   shuffle of the same slice of pos_in int32 [total]: for i = len-1 .. 1, j = mulhi32(word0 at counter (chain_id[c], epoch,
 *   0, i), i+1), swap elements i and j.  pos_off int32 [n_chain+1] (clamped to [0,total]; a pair with hi < lo is an empty
 *   list), chain_id int32 [n_chain].  One lane per chain; integer arithmetic only.  pos_in and perm_out must not overlap.
 * esmk_op_sample_rows: one token per row of logprobs fp32 [n,V], V <= 64.  row_chain / row_index int32 [n]: counter words 0
 *   and 3 of the row's uniform (word 1 = step).  The candidates are the bits of allowed_mask below V, minus the token
 *   exclude[i] (exclude int32 [n] or NULL; -1 or any value outside [0,V): none).  inv_temperature > 0: z_v = logprobs[v] *
 *   inv_temperature, m = max z, w_v = expf(z_v - m) over the candidates, added in fp32 in ascending token order; the token is
 *   the first candidate whose running sum exceeds u * total, the last candidate if none does; logq = z_tok - m - log(total),
 *   that value taken in fp64 from the fp32 inputs and rounded to fp32 once.
 *   inv_temperature == 0: the candidate with the largest logprobs, ties to the lowest index; logq = 0.  No candidate: token
 *   -1, logq 0.  A row whose candidates all hold -inf (no log_softmax of finite logits gives one) has no distribution: with
 *   inv_temperature > 0 it returns the last candidate and logq = NaN, greedy the lowest candidate.  token_out int32 [n],
 *   logq_out fp32 [n], u_out fp32 [n] or NULL.
 * esmk_op_commit_tokens: tokens[slot[i], pos[i]] = token[i] on tokens int64 [B,T]; slot, pos, token int32 [n].  A row with
 *   token < 0 or a position outside [0,T) writes nothing; a slot outside [0,B) is clamped.  The (slot, pos) pairs of one
 *   call must be distinct.
 * esmk_op_sample_rows_ex: esmk_op_sample_rows with a top-k / nucleus filter in front of the draw and a per-row score.  The
 *   candidates are as above.  Candidate v RANKS before w when logprobs[v] > logprobs[w], or they are equal and v < w; NaN
 *   ranks last.  The rank comes from the fp32 inputs (inv_temperature > 0, so it is the order of the tempered values): exact
 *   comparison logic.  w_v = expf(z_v - m) as above; E_r = the fp32 sum of the weights of the ranks before r, added in rank
 *   order, W = that sum over all candidates.  The candidate of rank r is KEPT when (top_k == 0 || r < top_k) && (top_p >= 1 ||
 *   E_r < top_p * W); rank 0 is always kept.  top_k == 0 and top_p == 1 switch the filters off outright: no such arithmetic,
 *   kept = the candidates, and token, logq and u are the bits of esmk_op_sample_rows.  The draw runs as above over the kept
 *   set: fp32 running sums in ascending token order, the first kept token whose sum exceeds u * total (the last kept one if
 *   none does), logq in fp64 relative to the kept set, rounded once.  Greedy (inv_temperature == 0) ignores the filters — the
 *   argmax is rank 0 — and computes kept and the score with z = logprobs.  kept_out uint64 [n] or NULL: the kept bitset (0:
 *   no candidate).  The score is taken over the candidates BEFORE filtering, q = softmax(z): score_kind 1 (confidence) = max
 *   log q, 2 (negative entropy) = sum of q log q with the terms of q == 0 counted as 0, both in fp64 from the fp32 inputs and
 *   rounded to fp32 once; 0 = none (score_out_dev may be NULL and is not written).  No candidate: score = -inf.  A row whose
 *   candidates all hold -inf has NaN weights: with top_p < 1 only rank 0 is kept, and logq and the score are NaN.
 * esmk_op_select_rows: the per-chain choice of the best rows.  Chain c owns the rows [row_off[c], row_off[c+1]) of score fp32
 *   [n] (row_off int32 [n_chain+1], clamped to [0,n]; a pair with hi < lo is an empty list).  k_c = clamp(sel_off[c+1] -
 *   sel_off[c], 0, len_c).  sel_out[sel_off[c] ..] receives the row indices (into score) of the k_c rows of the chain with the
 *   largest score, best first: equal scores go to the lower row, NaN ranks below everything including -inf, among NaNs the
 *   lower row first.  rest_out[rest_off[c] ..] receives the other rows of the chain in ascending row order, at most
 *   rest_off[c+1] - rest_off[c] of them.  sel_off, rest_off int32 [n_chain+1]; sel_out int32 [n_sel], rest_out int32 [n_rest];
 *   elements outside every slice are left untouched and nothing is written outside [0,n_sel) / [0,n_rest) whatever the
 *   offsets hold.  One workgroup per chain counts ranks (len_c^2 comparisons: no sort, no scratch) and compacts the rest list
 *   in order.  Comparison logic only: the result is exact and does not depend on the launch.  n_rest may be 0, with
 *   rest_off_dev and rest_out_dev NULL: no rest list.
 * Refused before any HIP call: null pointers (exclude_dev, u_out_dev, kept_out_dev may be NULL; score_out_dev when score_kind
 * == 0), n_chain, total, n, B or T <= 0, V outside 1 .. 64, a negative epoch or step, an inv_temperature that is negative or
 * not finite, n or B*T > 2^24, top_k outside 0 .. 64, a top_p outside (0, 1] or not finite, score_kind outside 0 .. 2; for
 * esmk_op_select_rows n_chain, n or n_sel outside 1 .. 2^24, n_rest outside 0 .. 2^24. */
int esmk_op_permute_positions(const int32_t* pos_off_dev, const int32_t* pos_in_dev, const int32_t* chain_id_dev,
                              int32_t* perm_out_dev, int n_chain, int total, uint64_t seed, int epoch, void* stream);
int esmk_op_sample_rows(const float* logprobs_dev, const int32_t* row_chain_dev, const int32_t* row_index_dev,
                        const int32_t* exclude_dev, uint64_t allowed_mask, float inv_temperature, uint64_t seed, int step,
                        int32_t* token_out_dev, float* logq_out_dev, float* u_out_dev, int n, int V, void* stream);
int esmk_op_commit_tokens(int64_t* tokens_dev, const int32_t* row_chain_slot_dev, const int32_t* pos_dev,
                          const int32_t* token_dev, int n, int B, int T, void* stream);
int esmk_op_sample_rows_ex(const float* logprobs_dev, const int32_t* row_chain_dev, const int32_t* row_index_dev,
                           const int32_t* exclude_dev, uint64_t allowed_mask, float inv_temperature, uint64_t seed, int step,
                           int top_k, float top_p, int score_kind, int32_t* token_out_dev, float* logq_out_dev, float* u_out_dev,
                           float* score_out_dev, uint64_t* kept_out_dev, int n, int V, void* stream);
int esmk_op_select_rows(const float* score_dev, const int32_t* row_off_dev, const int32_t* sel_off_dev,
                        const int32_t* rest_off_dev, int32_t* sel_out_dev, int32_t* rest_out_dev, int n_chain, int n, int n_sel,
                        int n_rest, void* stream);

/* Metropolis-Hastings design toward a target contact map (esm_amd/design.py; csrc/design.hip).  The state of a chain is its token
 * row and its current energy E = w_contact * E_contact + w_lm * E_lm, both on the device.  A step with the uniform proposal is
 *   esmk_op_propose_mutations -> esmk_op_substitute_rows -> esmk_forward_rows_contacts (the residue rows of every proposal
 *   selected) -> esmk_op_sum_target_rows -> esmk_op_contact_energy -> esmk_op_mh_accept
 * and with the LM proposal
 *   esmk_op_propose_mutations (the site) -> esmk_op_mask_rows_multi -> esmk_forward_rows (the masked site's row) ->
 *   esmk_op_sample_rows at counter (chain, step, 1, site) -> esmk_op_hastings_rows -> esmk_op_substitute_rows -> ... as above
 * on one stream; the host reads nothing in between.  Philox as in the sampling section, counter (chain id, step, purpose, 0):
 * purpose 2 = proposal (word 0: the site, word 1: the token), purpose 3 = acceptance.  No atomics; all list data is device data.
 * esmk_op_propose_mutations: one lane per chain c.  site = pos[pos_off[c] + mulhi32(word0, len_c)], pos_off int32 [n_chain+1]
 *   (clamped to [0,total]; a pair with hi < lo is an empty list), pos int32 [total].  old = tokens[slot[c], site] (tokens int64
 *   [B,T]; slot int32 [n_chain] clamped to [0,B), or NULL: slot c).  The candidates are the bits of allowed_mask below V, minus
 *   old when force_new; tok = the set bit number mulhi32(word1, n_cand) of the candidates in ascending token order.  An empty
 *   list or a site outside [0,T): site = old = tok = -1.  No candidate: tok = -1.  Integer arithmetic only.
 * esmk_op_contact_energy: contacts fp32 [B,S,S] probabilities, target uint8 [S,S] (0 = no contact, 1 = contact, 2 = ignore).
 *   Only pairs i < j with j - i >= min_sep (>= 1) and target != 2 count.  p is clamped to [2^-24, 1 - 2^-24] and taken to fp64.
 *   kind 0 ("pos"): energy = -mean over the counted target contacts of log p, count = their number; kind 1 ("bce"): energy =
 *   -mean over the counted pairs of y log p + (1 - y) log(1 - p), count = their number.  One workgroup of 256 lanes per chain;
 *   lane t adds the terms of the elements t, t + 256, ... of the row-major map in that order, the lane sums are added in a
 *   butterfly per wavefront and the four wavefront sums in order: the order of addition depends on S, min_sep and the target
 *   alone.  energy_out fp64 [B], count_out int32 [B]; a count of 0 gives energy 0.0.
 * esmk_op_mh_accept: one lane per chain, fp64, every operation rounded once (no fused multiply-add).  E' = w_contact *
 *   e_contact[c] + w_lm * (-(lp_sum[c] / n_res[c])): e_contact fp64 [n_chain] or NULL (0), lp_sum fp64 [n_chain]
 *   (esmk_op_sum_target_rows over the chain's residue rows) or NULL (0), n_res int32 [n_chain] (<= 0: the LM term is 0).
 *   dE = E' - e_cur[c]; h = hastings[c] or 0 (NULL); u = (word0 >> 8) * 2^-24 at counter (chain_id[c], step, 3, 0).  Accept iff
 *   tok[c] >= 0 and (a >= 0 or u < exp(a)), a = -dE * inv_temperature + h; inv_temperature == +inf (greedy): iff tok[c] >= 0 and
 *   dE <= 0.  On acceptance tokens[slot[c], site[c]] = tok[c] (slot as above; a site outside [0,T) writes no token), e_cur[c] =
 *   E', and e_contact_cur[c] / e_lm_cur[c] (fp64 [n_chain] or NULL) receive the components.  accepted_out uint8 [n_chain];
 *   u_out, e_prop_out fp64 [n_chain] or NULL: written for every chain.
 * esmk_op_hastings_rows: h_out fp64 [n], h[c] = (double)inv_t_prop * ((double)logprobs[c, old[c]] - (double)logprobs[c, new[c]]),
 *   logprobs fp32 [n,V]: the log ratio of the reverse and the forward LM proposal, which share the context and the candidate
 *   set.  old or new outside [0,V): 0.
 * Refused before any HIP call: null pointers (slot_dev, e_contact_dev, lp_sum_dev with n_res_dev, hastings_dev,
 * e_contact_cur_dev, e_lm_cur_dev, u_out_dev, e_prop_out_dev may be NULL), n_chain, n, B, T or S <= 0, total < 0, V outside
 * 1 .. 64, S > 32768, B*T, n_chain or n > 2^24, min_sep < 1, kind outside 0 .. 1, a negative step, an inv_temperature that is
 * negative or NaN, weights that are not finite, an inv_t_prop that is negative or not finite. */
int esmk_op_propose_mutations(const int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* pos_off_dev, const int32_t* pos_dev,
                              const int32_t* chain_id_dev, uint64_t allowed_mask, int force_new, uint64_t seed, int step,
                              int32_t* site_out_dev, int32_t* old_out_dev, int32_t* tok_out_dev, int n_chain, int B, int T, int total,
                              int V, void* stream);
int esmk_op_contact_energy(const float* contacts_dev, const uint8_t* target_dev, double* energy_out_dev, int32_t* count_out_dev, int B,
                           int S, int min_sep, int kind, void* stream);
int esmk_op_mh_accept(int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* site_dev, const int32_t* tok_dev,
                      const int32_t* chain_id_dev, const double* e_contact_dev, const double* lp_sum_dev, const int32_t* n_res_dev,
                      const double* hastings_dev, double w_contact, double w_lm, double inv_temperature, uint64_t seed, int step,
                      double* e_cur_dev, double* e_contact_cur_dev, double* e_lm_cur_dev, uint8_t* accepted_out_dev, double* u_out_dev,
                      double* e_prop_out_dev, int n_chain, int B, int T, void* stream);
int esmk_op_hastings_rows(const float* logprobs_dev, const int32_t* old_dev, const int32_t* new_dev, float inv_t_prop,
                          double* h_out_dev, int n, int V, void* stream);

/* The n-gram term of the design energy and replica exchange (esm_amd/design.py; csrc/tempering.hip).  fp64, every operation rounded
 * once (no fused multiply-add), no atomics.
 * esmk_op_ngram_energy: lm-design's n-gram term (examples/lm-design/utils/ngram.py, compute_kl_div).  tokens int64 [B,T]; the S
 *   residues of a chain are the positions first .. first + S - 1; code int32 [V] maps a token to 0 .. A-1 or to -1 (a token outside
 *   [0,V), or a code outside [0,A), counts as -1).  order_mask: bit n-1 chooses order n = 1 .. 4; qn_dev fp64 [A^n] is the dense
 *   background table of order n, every entry finite and positive (the caller has applied the floor).  Per chain and chosen order:
 *   window i (0 <= i <= S-n) is valid iff its n codes are all >= 0, its key is sum_k code[i+k] * A^(n-1-k); total = the valid
 *   windows, c_i = the valid windows with the key of window i, window i is a first window iff no valid j < i has its key; KL_n =
 *   the sum over the first windows of p * log(p / qn[key]), p = c_i / total; total == 0 (S < n included): KL_n = 0.0.
 *   energy_out fp64 [B] = (((0.0 + KL_a) + KL_b) + ...) over the chosen orders, ascending.  One workgroup of 256 lanes per chain:
 *   lane t adds the terms of the first windows among t, t + 256, ... in that order (any other window adds nothing), the lane sums
 *   are added in a butterfly per wavefront and the four wavefront sums in order: the order of addition depends on S and
 *   order_mask alone, and a chain gets the same bits alone and in any batch.  The counts are pairwise (S^2 comparisons per order).
 * esmk_op_mh_accept_ex: esmk_op_mh_accept with a temperature per chain and a third energy term.  inv_t fp64 [n_rung], rung int32
 *   [n_chain] or NULL (rung 0): chain c uses inv_t[clamp(rung[c], 0, n_rung-1)] (+inf: greedy, negative or NaN: rejects unless a
 *   >= 0 holds, as any NaN).  e_extra fp64 [n_chain] or NULL: E' = (w_contact * e_contact[c] + w_lm * e_lm) + w_extra * e_extra[c];
 *   with e_extra NULL the last addition is not made, and that call with one rung gives the bits of esmk_op_mh_accept.  On
 *   acceptance e_extra_cur[c] (fp64 [n_chain] or NULL) = e_extra[c].  Counter, rule and the other outputs: esmk_op_mh_accept.
 * esmk_op_replica_swap: chains form ladders of K consecutive slots (ladder l: slots l*K .. l*K+K-1); rung int32 [n_ladder*K]
 *   holds a permutation of 0 .. K-1 per ladder, inv_t fp64 [K].  In swap round r one lane per pair (ladder l, lower rung k), k % 2
 *   == r % 2 and k+1 < K, scans the ladder's K slots for the chain x at rung k and the chain y at rung k+1, computes a = (inv_t[k]
 *   - inv_t[k+1]) * (e_cur[x] - e_cur[y]) and u = (word0 >> 8) * 2^-24 at Philox counter (ladder_id[l], r, 4, k) — purpose 4 = swap,
 *   next to 0 .. 3 — and accepts iff a >= 0 or u < exp(a) (a NaN rejects): rung[x] = k+1, rung[y] = k.  Temperatures move, sequences
 *   and chain ids stay with their slots.  The pairs of a round are disjoint: plain stores.  accepted_out uint8 [n_ladder*K]: 1 for
 *   both chains of an accepted pair, else 0; u_out fp64 [n_ladder*K]: the pair's u for both chains of an attempted pair, -1.0
 *   elsewhere.  inv_t_host: the caller's host copy of inv_t, read for validation only.
 * Refused before any HIP call: null pointers (slot_dev, e_contact_dev, lp_sum_dev with n_res_dev, hastings_dev, e_extra_dev,
 * rung_dev of esmk_op_mh_accept_ex, the *_cur_dev components, u_out_dev and e_prop_out_dev of esmk_op_mh_accept_ex, and the table of
 * an order that is not chosen may be NULL), B, T, S, n_chain, n_ladder or n_rung <= 0, B*T, n_chain, n_rung or n_ladder*K > 2^24,
 * S > 32768, first < 0 or first + S > T, V outside 1 .. 64, A outside 1 .. 32, an order_mask without one of the bits 0 .. 3 or
 * with another bit, a chosen order whose table is NULL, weights that are not finite, a negative step or round, K outside 1 .. 64,
 * an inv_t_host entry that is negative, NaN or infinite (a ladder has no greedy rung). */
int esmk_op_ngram_energy(const int64_t* tokens_dev, const int32_t* code_dev, const double* q1_dev, const double* q2_dev,
                         const double* q3_dev, const double* q4_dev, int order_mask, double* energy_out_dev, int B, int T, int first,
                         int S, int V, int A, void* stream);
int esmk_op_mh_accept_ex(int64_t* tokens_dev, const int32_t* slot_dev, const int32_t* site_dev, const int32_t* tok_dev,
                         const int32_t* chain_id_dev, const double* e_contact_dev, const double* lp_sum_dev, const int32_t* n_res_dev,
                         const double* hastings_dev, const double* e_extra_dev, double w_contact, double w_lm, double w_extra,
                         const double* inv_t_dev, const int32_t* rung_dev, int n_rung, uint64_t seed, int step, double* e_cur_dev,
                         double* e_contact_cur_dev, double* e_lm_cur_dev, double* e_extra_cur_dev, uint8_t* accepted_out_dev,
                         double* u_out_dev, double* e_prop_out_dev, int n_chain, int B, int T, void* stream);
int esmk_op_replica_swap(int32_t* rung_dev, const double* e_cur_dev, const double* inv_t_dev, const double* inv_t_host,
                         const int32_t* ladder_id_dev, uint64_t seed, int round, uint8_t* accepted_out_dev, double* u_out_dev,
                         int n_ladder, int K, void* stream);

/* Choosing the rows of an MSA on the device (esm_amd/msa_select.py; csrc/msa_select.hip).  An MSA is msa uint8 [N,ld], row-major:
 * L <= ld columns count, bytes in [L,ld) of a row are never counted whatever they hold, and every byte value 0 .. 255 is legal
 * (a gap is a byte like any other).  mism(i,j) = #{c < L : msa[i,c] != msa[j,c]}.  Integer arithmetic and comparison logic
 * only, so every result is exact and none depends on the launch geometry; the race keys are one fp64 product each.
 * esmk_op_msa_mismatch_rows: out int32 [nq,N], out[q,j] = mism(query[q], j); query int32 [nq] is device data, an index outside
 *   [0,N) is clamped.  One wavefront per pair.
 * esmk_op_msa_neighbor_counts: count_out int32 [N], count[i] = #{j in [0,N) : mism(i,j) <= max_mismatch}, j = i included; a
 *   negative max_mismatch gives all zeros.  The N^2 L hot path: 64 x 64 tiles of row pairs, the columns staged through LDS in
 *   chunks of 128, 4 x 4 pairs per lane in registers, four columns per dword compare, the tail past L masked.  Every pair is
 *   computed from both sides; count_out is zeroed on the stream and receives one integer atomic add per row and workgroup.
 * esmk_op_msa_greedy_select: sel_out int32 [num]: sel[0] = first; for k = 1 .. num-1, S_k[j] = sum over t < k of mism(sel[t], j)
 *   and sel[k] = the not-yet-selected j with the largest (mode 0) or smallest (mode 1) S_k[j], ties to the lowest j.  Integer
 *   sums; the steps run back to back on the stream, step k reads sel[k-1] on the device and the host reads nothing in
 *   between.  sum_work int32 [N] is the caller's scratch.
 * esmk_op_msa_race_keys: key_out fp64 [N], key_i = -log(u_i) * count_i in fp64, u_i = (word0 >> 8) * 2^-24 with word0 the first
 *   Philox4x32-10 word under the key seed at counter (subsample, 0, 2, i): purpose 2, next to the sampler's 0 and 1.  count
 *   int32 [N] or NULL (all ones); u_i == 0 or count_i <= 0 gives +inf.  The rows of the smallest keys are a draw without
 *   replacement with weights 1 / count.
 * esmk_op_rank_keys: rank_out int32 [N], rank_i = #{j : key_j < key_i, or key_j == key_i and j < i}; NaN ranks after
 *   everything, among NaNs the lower index first: a permutation of 0 .. N-1.  N^2 comparisons, no sort.
 * Refused before any HIP call: null pointers (count_dev may be NULL), N, L or nq <= 0, ld < L, N*ld >= 2^31, L > 65535, nq*N >=
 * 2^31, num outside 1 .. N, first outside [0,N), num*L >= 2^31, mode outside 0 .. 1, a negative subsample, and for the last two
 * entries N > 2^24. */
int esmk_op_msa_mismatch_rows(const uint8_t* msa_dev, int N, int L, int ld, const int32_t* query_dev, int nq, int32_t* out_dev,
                              void* stream);
int esmk_op_msa_neighbor_counts(const uint8_t* msa_dev, int N, int L, int ld, int max_mismatch, int32_t* count_out_dev,
                                void* stream);
int esmk_op_msa_greedy_select(const uint8_t* msa_dev, int N, int L, int ld, int first, int num, int mode, int32_t* sum_work_dev,
                              int32_t* sel_out_dev, void* stream);
int esmk_op_msa_race_keys(const int32_t* count_dev, int N, uint64_t seed, int subsample, double* key_out_dev, void* stream);
int esmk_op_rank_keys(const double* key_dev, int32_t* rank_out_dev, int N, void* stream);

/* The categorical Jacobian of one protein (esm_amd/jacobian.py): every candidate token t_a of a list of nA <= 32 put at every
 * residue position p_i of ONE sequence, J[i,a,j,b] = logits(copy(i,a))[p_j, t_b] - logits(x)[p_j, t_b], fp32 [L,nA,L,nA] — the
 * fp32 difference of two fp32 logits.  A chunk of copies is esmk_op_substitute_rows -> esmk_forward_rows (the L residue rows of
 * every copy selected) -> esmk_op_jacobian_scatter on one stream; the host reads nothing in between, and J stays on the
 * device: esmk_op_jacobian_center, esmk_op_jacobian_contacts and esmk_op_apc turn it into an [L,L] contact map there.  No
 * atomics; every sum is fp64 in a fixed order, so no result depends on the launch geometry or on how the copies were chunked.
 * Every index into J is 64 bit (the 1600 L^2 bytes of 20 candidates pass 2^31 at L = 1159).
 * esmk_op_substitute_rows: out int64 [n,T], row i = tokens[src_row[i], :] (tokens int64 [B,T]; src_row int32 [n] or NULL = row
 *   0) with position pos[i] replaced by tok[i] (int32 [n] each).  All lists are device data: a source row outside [0,B) is
 *   clamped, a position outside [0,T) or a token outside [0,V) substitutes nothing.
 * esmk_op_jacobian_scatter: out[c,j,b] = logits[c*L + j, cols[b]] - wt[j, cols[b]] for the n_copies copies of a chunk; logits
 *   fp32 [n_copies*L, V], wt fp32 [L,V], cols int32 [nA] (device data, clamped to [0,V)), out = J + copy0*L*nA, the slice of J
 *   at the chunk's first copy (copy c = i*nA + a).
 * esmk_op_jacobian_center: Jc = (P_i x P_a x P_j x P_b) J, P = I - 11'/n along that axis, as four passes IN PLACE in the order
 *   b, j, a, i.  In every pass the mean of a line is the fp64 sum of its fp32 values in ascending index order, divided by n, and
 *   every element becomes (float)((double)x - mean): one rounding per pass.  One lane owns a line; the lanes of a wavefront
 *   run along the contiguous index.
 * esmk_op_jacobian_contacts: S_out fp32 [L,L], S[i,j] = sqrt(sum over (a,b) of (0.5 (Jc[i,a,j,b] + Jc[j,b,i,a]))^2): the terms
 *   in fp64, lane l of one wavefront per pair i <= j adding the terms l, l + 64, ... (index a*nA + b) by fused multiply-add, the
 *   64 partial sums added in a butterfly, the fp64 square root rounded to fp32 once and stored to S[i,j] and S[j,i]: S is
 *   symmetric bit for bit.
 * esmk_op_apc: in place on S fp32 [L,L]: S[i,i] = 0; C[i,j] = (float)((double)S[i,j] - r_i * c_j / s) with r, c, s the row,
 *   column and total sums of S (diagonal as zero) in fp64; s == 0: S stays (diagonal zero); C[i,i] = 0.  work_dev: 2 L + 1
 *   doubles of scratch (r, c, s), the caller's.
 * Refused before any HIP call: null pointers (src_row_dev may be NULL), L, nA, n, n_copies, B, T or V <= 0, nA > 32,
 * L*nA*L*nA >= 2^40, L*nA, n_copies*L, B*T or n*T > 2^24, n_copies > L*nA. */
int esmk_op_substitute_rows(const int64_t* tokens_dev, const int32_t* src_row_dev, const int32_t* pos_dev, const int32_t* tok_dev,
                            int64_t* out_dev, int B, int T, int n, int V, void* stream);
int esmk_op_jacobian_scatter(const float* logits_dev, const float* wt_dev, const int32_t* cols_dev, float* out_dev, int n_copies,
                             int L, int nA, int V, void* stream);
int esmk_op_jacobian_center(float* J_dev, int L, int nA, void* stream);
int esmk_op_jacobian_contacts(const float* Jc_dev, float* S_out_dev, int L, int nA, void* stream);
int esmk_op_apc(float* S_dev, double* work_dev, int L, void* stream);

/* The token front end — the kernels that turn tokens into the layer-0 activation and into the bookkeeping every later kernel
 * trusts — one launch at a time (tests/test_frontend_ops_gpu.py).  Validation, then the launchers the engines call.  Refused
 * before any HIP call: null pointers (the ones named optional below may be NULL), B, T, R, C, n, rows, N, vocab or npos <= 0,
 * E / D not a positive multiple of 4, a bad segment table.  Segment tables (segments_host int32 [n_seg][2] = (first row,
 * length)) follow the rules of esmk_forward_packed — rows % 64 == 0, the first segment starts at row 0, starts ascending
 * multiples of 16, segments disjoint, lengths > 0, inside rows — and are host arrays: the entry uploads them, waits for the
 * stream and frees the copy.
 * esmk_op_seq_stats (esm2.py:82,86-92,108-109; multihead_attention.py:368-374): tokens int64 [B,T] -> scale fp32 [B] =
 *   1 - n_mask / n_nonpad (NaN for a row of padding only), key_bias fp32 [B,T] = 0 / -inf, seq_info int32 [B,2] = (#pads,
 *   1 + index of the last non-pad token; 0 when there is none), keep fp32 [B,T] = 1 - pad (optional).  token_dropout is
 *   the launcher's argument of that name: the statistics do not depend on it.
 * esmk_op_packed_stats: the same per segment of a packed row space, tokens int64 [rows]: scale_row, key_bias, keep (optional)
 *   fp32 [rows], row_pos int32 [rows] = row - segment start, seg_npad int32 [n_seg]; rows outside every segment get
 *   (1, -inf, 0, 0).
 * esmk_op_zero_gap_rows: rows outside every segment of buf [rows][row_bytes] := 0; row_bytes a positive multiple of 16.
 * esmk_op_embed (esm2.py:84-95): x fp32 [B,T,E] = table[tok] (a zero row for tok outside [0,vocab)); with token_dropout
 *   <mask> rows are zeroed and every row becomes (x * fp32(0.88)) / scale[b]; <pad> rows are zeroed.  The packed engine
 *   calls it as B = rows, T = 1 with the per-row scale of esmk_op_packed_stats.  scale may be NULL without token_dropout.
 * esmk_op_embed_esm1 (esm1.py:123-133): x = embed_scale * table[tok], token dropout as above, + sinus[t] (fp32 [T,E]) on
 *   non-pad tokens; pad rows are NOT zeroed.
 * esmk_op_add_positions (modules.py:240-257): x[b,t,:] += pos_emb[min(cumsum(nonpad)[t] * nonpad[t] + pad_idx, npos - 1)],
 *   pos_emb fp32 [npos,E].  segments_host NULL: tokens [B,T]; n_seg and rows must be 0.  Otherwise tokens [rows], segment s
 *   is a sequence, B = n_seg and T >= the longest segment (the engine passes the longest); rows outside every segment are not
 *   touched.  T must not exceed npos - pad_idx - 1 (the engine's rule), and (T + 4) * 4 bytes must fit the default dynamic
 *   LDS limit of 64 KiB.
 * esmk_op_scale_rows (esm1.py:138-139): x fp32 [rows,E] row r *= keep[r].
 * esmk_op_msa_embed (msa_transformer.py:152-165): tokens int64 [B,R,C] -> x fp32 [B,R,C,D] = (tok_emb[tok] + pos_emb[p]) +
 *   msa_pos[r] (msa_pos fp32 [R,D], optional), keep fp32 [B,R,C] = 1 - pad, col_fill fp32 [B,C,R] = pad, any_pad int32 [1] =
 *   1 iff the batch holds a pad (reset by every call).  C <= npos - pad_idx - 1; (C + 4) * 4 bytes of dynamic LDS as above.
 * esmk_op_sinus_table (modules.py:283-295): table fp32 [T, 2 half], row t = sin | cos of fp32(pos0 + t) * freq[i], precise
 *   sinf / cosf.  esmk_op_rope_table (rotary_embedding.py:47-61): cos, sin fp32 [T,half] of fp32(t) * inv_freq[i].
 *   T * half < 2^31.
 * esmk_op_gather_rows: out fp32 [n,E] = x[clamp(sel[i], 0, N - 1)], x fp32 [N,E], sel int32 [n] (device data, hence the
 *   clamp). */
int esmk_op_seq_stats(const int64_t* tokens_dev, int B, int T, int pad_idx, int mask_idx, int token_dropout, float* scale_dev,
                      float* key_bias_dev, int32_t* seq_info_dev, float* keep_dev, void* stream);
int esmk_op_packed_stats(const int64_t* tokens_dev, const int32_t* segments_host, int n_seg, int rows, int pad_idx,
                         int mask_idx, float* scale_row_dev, float* key_bias_dev, int32_t* row_pos_dev, int32_t* seg_npad_dev,
                         float* keep_dev, void* stream);
int esmk_op_zero_gap_rows(void* buf_dev, const int32_t* segments_host, int n_seg, int rows, size_t row_bytes, void* stream);
int esmk_op_embed(const int64_t* tokens_dev, const float* table_dev, const float* scale_dev, float* x_dev, int B, int T, int E,
                  int vocab, int pad_idx, int mask_idx, int token_dropout, void* stream);
int esmk_op_embed_esm1(const int64_t* tokens_dev, const float* table_dev, const float* scale_dev, const float* sinus_dev,
                       float* x_dev, int B, int T, int E, int vocab, int pad_idx, int mask_idx, int token_dropout,
                       float embed_scale, void* stream);
int esmk_op_add_positions(const int64_t* tokens_dev, const float* pos_emb_dev, float* x_dev, int B, int T, int E, int pad_idx,
                          int npos, const int32_t* segments_host, int n_seg, int rows, void* stream);
int esmk_op_scale_rows(float* x_dev, const float* keep_dev, int rows, int E, void* stream);
int esmk_op_msa_embed(const int64_t* tokens_dev, const float* tok_emb_dev, const float* pos_emb_dev, const float* msa_pos_dev,
                      float* x_dev, float* keep_dev, float* col_fill_dev, int32_t* any_pad_dev, int B, int R, int C, int D,
                      int vocab, int pad_idx, int npos, void* stream);
int esmk_op_sinus_table(const float* freq_dev, float* table_dev, int T, int half, int pos0, void* stream);
int esmk_op_rope_table(const float* inv_freq_dev, float* cos_dev, float* sin_dev, int T, int half, void* stream);
int esmk_op_gather_rows(const float* x_dev, const int32_t* sel_dev, float* out_dev, int N, int E, int n, void* stream);

/* ContactPredictionHead.forward (modules.py:338-357) incl. symmetrize/apc (modules.py:27-41).
 * attn fp32 [B,C=L*H,T,T]; w fp32 [C]; b fp32 [1]; scratch fp32 >= B*C*(T+1) floats;
 * out fp32 [B,T-2,T-2] (crop follows prepend_bos/append_eos). */
int esmk_op_contacts(const float* attn_dev, const int64_t* tokens_dev, const float* w_dev,
                     const float* b_dev, float* scratch_dev, float* out_dev, int B, int C, int T,
                     int eos_idx, int prepend_bos, int append_eos, void* stream);

/* Linear pairwise heads on the attention maps without the [B,L,H,T,T] tensor (csrc/pair_head.hip; esm_amd/pair_head.py).  The
 * head of lm-design's structure model (examples/lm-design/utils/linear_projection.py:85-135) is two 1 x 1 convolutions over the
 * C = L*H attention channels c = layer * H + head: n_sym outputs on the symmetrised maps P + P^T, n_asym on the maps as they are.
 * With w fp32 [C][n_sym + n_asym] (row c = the weights of channel c, the n_sym symmetric outputs first) and bias [n_sym + n_asym]:
 *   Z[b,i,j,o]   = sum over c ascending of w[c,o] * P_c[b,i,j]          (fp32, one fused multiply-add per channel)
 *   out[b,i,j,o] = Z[b,i,j,o] + Z[b,j,i,o] + bias[o]  for o < n_sym,    Z[b,i,j,o] + bias[o]  for the rest
 * out fp32 [B,S,S,n_sym + n_asym], S = T - prepend_bos - append_eos: only the first / last position is cropped (no <eos> mask,
 * no APC, linear_projection.py:76-82).  P_c is recomputed from the q, k and row log-sum-exp the attention kernel of the layer
 * used; rows and columns of <pad> tokens are exact zeros, so entries that involve a <pad> position hold the bias.  One writer
 * per element, no atomics, a fixed order of addition: a sequence's map does not depend on the batch it ran in.
 * esmk_set_pair_head: the handle keeps a device copy of w_host / bias_host (host arrays); n_sym = n_asym = 0 clears the head.
 *   Refused before any HIP call: a null model, an MSA handle, negative counts, n_sym + n_asym > 64, null arrays with a head.
 * esmk_forward_rows_pair: esmk_forward_rows (the layer stack once, head and log-softmax on the n_sel selected rows; n_sel = 0
 *   with null row arguments is allowed) plus pair_out_dev; every layer's q, k and lse are kept in the workspace
 *   (esmk_rows_pair_workspace_bytes: 2 L B T H slots operand elements + 4 L B H T bytes on top of esmk_forward_rows') and the
 *   head runs as ONE launch over all channels after the last layer.  The log-probability rows are bit for bit those of
 *   esmk_forward_rows.  Padded batches only; every model and precision mode esmk_forward_rows_contacts serves; the handle's
 *   stream edits apply.  Refused: no head set, an MSA handle, T - prepend_bos - append_eos <= 0, what esmk_forward_rows refuses.
 * esmk_op_pair_head: the two kernels on caller-supplied stacked operands, laid out as the padded case of
 *   esmk_op_contacts_fused_ex: q, k [L,B,H,T,head_dim] operand dtype (q in the log2 domain), lse fp32 [L,B,H,T] (log2 domain),
 *   key_bias fp32 [B,T] (0 / -inf) or NULL, tokens int64 [B,T] or NULL (either marks <pad>), w_dev / bias_dev device arrays
 *   (bias_dev may be NULL: 0), workspace of esmk_op_pair_head_workspace_bytes.
 * esmk_op_distogram_energy: lm-design's categorical cross-entropy (utils/loss.py:10-29) of the n_bins logits
 *   pair_logits[b,i,j,first .. first + n_bins) (fp32 [B,S,S,ld]) against target_bin uint8 [S,S]: per chain the mean over ALL
 *   ordered pairs (i,j) with target_bin[i,j] < n_bins (255 = ignore) and |i - j| >= min_sep of
 *   -log(softmax(inv_temp * logits)[target_bin] + 1e-8), in fp64.  One workgroup of 256 lanes per chain; lane t adds the terms of
 *   the elements t, t + 256, ... of the row-major map in that order, the lane sums in a butterfly per wavefront, the four
 *   wavefront sums in order: the order of addition does not depend on B.  energy_out fp64 [B], count_out int32 [B]; no counted
 *   pair: 0.0. */
int esmk_set_pair_head(esmk_model* m, const float* w_host, const float* bias_host, int n_sym, int n_asym);
int esmk_rows_pair_workspace_bytes(const esmk_model* m, int B, int T, int n_sel, size_t* bytes, size_t* logits_offset);
int esmk_forward_rows_pair(esmk_model* m, const void* packed_dev, const int64_t* tokens_dev, int B, int T,
                           const int32_t* sel_rows_dev, int n_sel, float* logprobs_out_dev, float* pair_out_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);
int esmk_op_pair_head_workspace_bytes(int H, int num_layers, size_t* bytes);
int esmk_op_pair_head(const void* q_dev, const void* k_dev, const float* lse_dev, const float* key_bias_dev,
                      const int64_t* tokens_dev, const float* w_dev, const float* bias_dev, int n_sym, int n_asym, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, int B, int H, int T, int num_layers, int head_dim, int pad_idx,
                      int prepend_bos, int append_eos, int operand_dtype, void* stream);
int esmk_op_distogram_energy(const float* pair_logits_dev, int ld, int first, int n_bins, const uint8_t* target_bin_dev, int B, int S,
                             int min_sep, double inv_temp, double* energy_out_dev, int32_t* count_out_dev, void* stream);

/* Sparse-autoencoder features of the residual stream (csrc/sae.hip; esm_amd/sae.py).  For a captured representation row x
 * (fp32 [E]):  u[e] = sub(mul(input_scale, x[e]), b_dec[e]) (two fp32 roundings, never fused);  z[f] = <w_enc[f], u> + b_enc[f];
 * feature f is ACTIVE iff z[f] > threshold[f], threshold >= 0 (a NaN is never active, +inf is); its activation is z[f] if active,
 * else 0.  The order everywhere is value descending, ties to the lower feature index; unused slots hold index -1 and value 0.
 * The product runs through esmk_op_linear (ESMK_EPI_STORE_F32) over the f16x3 operand images: the activation image written
 * here against the encoder image of esmk_op_split_weight_ex(parts = 3).  No entry uses a global atomic; every result is a
 * function of its inputs alone.  n = 0 is allowed everywhere (nothing is launched).
 * esmk_op_sae_rows: image fp16 [n, ld_image], row i = u of row rows[i] of x fp32 [N, ldx] (rows_dev int32 [n], clamped to
 *   [0, N - 1]: device data; NULL: row i, n <= N) as hi | hi | lo per 64-column K tile, hi = fp16(u), lo = fp16(u - hi): the
 *   layout esmk_op_layernorm_ex(x3 = 1) writes, 3 Ep columns with Ep = E rounded up to 64, pad columns zero; columns behind
 *   3 Ep are not written.  b_dec_dev fp32 [E] or NULL (zeros).  |u| must stay inside fp16's range.
 *   Refused: null x / image, E % 4, ldx < E or ldx % 4, ld_image < 3 Ep or ld_image % 4, a non-finite input_scale, n > N
 *   without a list, x / b_dec not 16-byte aligned.
 * esmk_op_sae_topk: one workgroup per row of z fp32 [n, ldz]: n_active[i] = the number of active features (k_sae > 0, a
 *   top-k autoencoder that keeps k_sae features per row: min(k_sae, that number)), indices int32 [n, k] / values fp32 [n, k] =
 *   the k best.  threshold_dev fp32 [F] or NULL (then the scalar `threshold`).  Rows with at most esmk_op_sae_cand() actives
 *   are compacted into LDS and sorted there; rows with more go through a radix select over the row first (8-bit digits of the
 *   64-bit key (value bits << 32) | (0xFFFFFFFF - index) from the high digit down) — path_dev int32 [n] or NULL receives 0 for
 *   the first path and the number of digit passes for the second.  cutoff_dev uint64 [n] or NULL: the key of the k_sae-th
 *   feature of a row with more than k_sae actives, else 0 (what esmk_op_sae_segment_max needs for a top-k autoencoder).
 *   Refused: null pointers, F outside 4 .. 65536 or F % 4, k outside 1 .. 256, k_sae outside 0, k .. 256, ldz < F or ldz % 4,
 *   a negative or NaN scalar threshold, z / threshold not 16-byte aligned.
 * esmk_op_sae_segment_max: protein_max fp32 [B, F] / protein_argmax int32 [B, F] updated IN PLACE (the caller starts them at
 *   0 / -1) from the chunk z fp32 [n, ldz] that holds rows row0 .. row0 + n of a row list; rows_dev int32 [n, 2] = the chunk's
 *   (sequence, position) pairs, seg_start_dev int32 [B + 1] = sequence b owns rows seg_start[b] .. seg_start[b + 1] of the
 *   WHOLE list.  One thread per (sequence, feature) walks the rows in order; a row replaces the stored value only if it is
 *   strictly greater (the lowest position wins ties; chunks in order on one stream merge a split sequence correctly).
 * esmk_op_sae_decode: out fp32 [n, E], out[e] = mul(inv_scale, b_dec[e] + sum over r = 0 .. k - 1 of mul(values[r],
 *   w_dec[indices[r], e])), one rounded product and one rounded add per term in rank order; indices outside [0, F) are
 *   skipped; w_dec fp32 [F, E], b_dec fp32 [E] or NULL (zeros). */
int esmk_op_sae_cand(void);
int esmk_op_sae_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, int n, const float* b_dec_dev, float input_scale,
                     void* image_dev, int ld_image, int E, void* stream);
int esmk_op_sae_topk(const float* z_dev, int ldz, const float* threshold_dev, float threshold, int n, int F, int k, int k_sae,
                     int32_t* indices_dev, float* values_dev, int32_t* n_active_dev, uint64_t* cutoff_dev, int32_t* path_dev,
                     void* stream);
int esmk_op_sae_segment_max(const float* z_dev, int ldz, const float* threshold_dev, float threshold, const uint64_t* cutoff_dev,
                            const int32_t* rows_dev, const int32_t* seg_start_dev, int row0, int n, int F, int B,
                            float* protein_max_dev, int32_t* protein_argmax_dev, void* stream);
int esmk_op_sae_decode(const int32_t* indices_dev, const float* values_dev, int n, int k, const float* w_dec_dev,
                       const float* b_dec_dev, float inv_scale, float* out_dev, int E, int F, void* stream);

/* Embedding-based alignment of two proteins (csrc/align.hip; esm_amd/align.py).  S[i][j] = <u_a[i], u_b[j]> is computed by
 * esmk_op_linear (ESMK_EPI_STORE_F32) over the two images of esmk_op_align_rows; on S, per pair (i, j over 0 .. La x 0 .. Lb,
 * fp32, H[0][0] = 0, E[i][0] = F[0][j] = -inf, max(x, y) = y if y > x else x, gap open o >= gap extend e >= 0):
 *     E[i][j] = max(H[i][j-1] - o, E[i][j-1] - e)       bit 2 of the cell's byte iff E[i][j-1] - e > H[i][j-1] - o
 *     F[i][j] = max(H[i-1][j] - o, F[i-1][j] - e)       bit 3, same rule
 *     H[i][j] = the first of maximal value among [stop = 0 (local mode only; global starts from -inf), D = S[i-1][j-1] +
 *               H[i-1][j-1], F[i][j], E[i][j]]           bits 0-1: 0, 1, 2, 3
 * Global (mode 0): score H[La][Lb], end cell (La, Lb).  Local (mode 1): the largest H, the end cell the first such cell in
 * row-major order; nothing above 0: score 0, end cell (0, 0).  No entry uses a global atomic; a pair's result does not depend
 * on the other pairs of the launch.  n_pairs = 0 / n = 0 is allowed everywhere (nothing is launched).
 * The pair table (int64 [n_pairs, 5], device data, every value clamped to the launch's buffers): first row of a in S, La,
 *   first column of b in S (a multiple of 8; the 8-aligned columns behind Lb must exist: n_cols is a multiple of 8), Lb, the
 *   pair's offset in the traceback buffer in bytes (a multiple of 8).  Byte (i, j), i, j >= 1, is at offset + (i - 1) * ld + j - 1
 *   with ld = Lb rounded up to 16; bytes of the columns behind Lb are 0.
 * esmk_op_align_panel: the columns a wavefront of the DP kernel covers at once; a longer side b goes panel by panel.
 * esmk_op_align_rows: image fp16 [n, ld_image] of rows rows[i] of x fp32 [N, ldx] (device data: an index beyond N - 1 is
 *   clamped, a NEGATIVE index writes a zero row; NULL: row i).  cosine = 1: u = x * r with r = float32(1 / sqrt(sum x^2)), the
 *   sum in fp64 (thread t of 256 adds the squares of columns 4 t .. 4 t + 3, 4 t + 1024 .., ascending; the partial sums fold as
 *   p[k] += p[k + s], s = 128, 64 .. 1), r = 0 for a zero row, the product rounded to fp32; cosine = 0: u = x (|x| < 65504).
 *   b_side = 0: hi | hi | lo per 64-column K tile, b_side = 1: hi | lo | hi (what esmk_op_split_weight_ex(parts = 3) writes).
 * esmk_op_align_enhance: in place, per pair block: S' = 0.5 ((S - mu_r[i]) inv_r[i] + (S - mu_c[j]) inv_c[j]), every operation
 *   rounded to fp32; mu = float32(fp64 sum in ascending index order / n), sigma = float32(sqrt(fp64 sum of (S - m)^2, ascending,
 *   / n)) with m the fp64 mean before rounding, inv = 1 / sigma in fp32, 0 where sigma = 0.  Pair blocks must not overlap.
 *   ws_dev: at least 2 max_lb floats (more lets more workgroups run: up to 1024 x 2 max_lb); max_lb bounds every Lb.
 * esmk_op_align_dp: score fp32 [n_pairs], end int32 [n_pairs, 2]; want_traceback = 1 also writes the bytes into tb_dev
 *   (tb_bytes long), want_traceback = 0 touches no byte buffer.  max_la / max_lb (1 .. 8192) bound every pair's sides.  When
 *   max_lb exceeds one panel, ws_dev must hold 2 (max_la + 1) floats per wavefront (at least one; up to 16384 are used).
 *   Refused: null pointers, a side bound outside 1 .. 8192, e < 0, e > o, non-finite penalties, n_cols % 8, ldS < n_cols or
 *   ldS % 4, S not 16-byte aligned, want_traceback without an 8-byte aligned buffer, a missing workspace.
 * esmk_op_align_traceback: one thread per pair walks from end[p] and writes the columns — (i, j) a match, (i, -1) residue i of
 *   a against a gap, (-1, j) — in ascending order into the BACK of the pair's slot of La + Lb columns: cols int32 [cols_cap, 2],
 *   slot_dev int64 [n_pairs] the slots' first columns; n_cols, n_match int32 [n_pairs], start int32 [n_pairs, 2] the cell the
 *   walk ended in.  At most La + Lb steps are taken whatever the bytes hold.
 * esmk_op_align_dp_ex / esmk_op_align_traceback_ex: the same with free end gaps.  free_ends (0 .. 15, mode 0 only; 0 is the
 *   plain entry): 1 a_start: H[i][0] = 0, the walk stops on column 0; 4 b_start: on row 0 the stop candidate is 0 (H[0][j] = 0,
 *   choice "stop"), the walk stops on row 0; 2 a_end: the cells (i, Lb), i = 1 .. La, are end-cell candidates next to the corner
 *   (La, Lb); 8 b_end: the cells (La, j), j = 1 .. Lb.  The largest H among the candidates wins, ties go to the lower row, then
 *   the lower column; cells with i = 0 or j = 0 are never candidates.  E and F on the borders, every fp32 operation and the
 *   byte layout are unchanged.  Refused before any HIP call: free_ends outside 0 .. 15, free_ends != 0 with mode 1.
 *   S_mask_dev (traceback_ex; NULL: none, and ldS = n_rows = n_cols = 0): the S of the DP call, writable, with its ldS, n_rows,
 *   n_cols: the walking thread stores -inf at S[i][j] of every MATCH column (i, j) of its path, inside the pair's block clamped
 *   to S and to the longest side (no table can direct a store outside S; for a table within the DP call's max_la / max_lb it is
 *   the block the DP read), so that the next esmk_op_align_dp_ex on the same S finds the pair's next best path (Waterman-Eggert;
 *   gap states may cross earlier paths).  A pair's block must belong to that pair alone: no pair listed twice, no overlapping
 *   blocks. */
int esmk_op_align_panel(void);
int esmk_op_align_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, int n, int cosine, int b_side, void* image_dev,
                       int ld_image, int E, void* stream);
int esmk_op_align_enhance(float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int max_lb,
                          float* ws_dev, long long ws_floats, void* stream);
int esmk_op_align_dp(const float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int mode,
                     float gap_open, float gap_extend, int max_la, int max_lb, float* score_dev, int32_t* end_dev, uint8_t* tb_dev,
                     long long tb_bytes, int want_traceback, float* ws_dev, long long ws_floats, void* stream);
int esmk_op_align_traceback(const int64_t* table_dev, int n_pairs, int mode, const int32_t* end_dev, const uint8_t* tb_dev,
                            long long tb_bytes, const int64_t* slot_dev, int32_t* cols_dev, long long cols_cap, int32_t* n_cols_dev,
                            int32_t* n_match_dev, int32_t* start_dev, void* stream);
int esmk_op_align_dp_ex(const float* S_dev, int ldS, int n_rows, int n_cols, const int64_t* table_dev, int n_pairs, int mode,
                        int free_ends, float gap_open, float gap_extend, int max_la, int max_lb, float* score_dev, int32_t* end_dev,
                        uint8_t* tb_dev, long long tb_bytes, int want_traceback, float* ws_dev, long long ws_floats, void* stream);
int esmk_op_align_traceback_ex(const int64_t* table_dev, int n_pairs, int mode, int free_ends, const int32_t* end_dev,
                               const uint8_t* tb_dev, long long tb_bytes, const int64_t* slot_dev, int32_t* cols_dev,
                               long long cols_cap, int32_t* n_cols_dev, int32_t* n_match_dev, int32_t* start_dev, float* S_mask_dev,
                               int ldS, int n_rows, int n_cols, void* stream);

/* Protein search on pooled embeddings (csrc/search.hip; esm_amd/search.py): one vector per protein, a cosine top-k against a
 * database of such vectors, the aligner above on the survivors.  The similarities are esmk_op_linear (ESMK_EPI_STORE_F32) over
 * the two cosine images of esmk_op_align_rows, block of database rows by block.  No entry uses a global atomic; a segment's /
 * a row's result does not depend on the other segments / rows of the launch.
 * esmk_op_pool_rows: out fp32 [n_seg, E]; out[s][e] = float32(sum / count), sum the fp64 sum of x[rows[r]][e] over
 *   r = seg_off[s] .. seg_off[s + 1] - 1 in ascending r, count the number of those r; an empty segment gives a zero row
 *   (esmk_op_align_rows turns a zero row into a zero unit vector), not NaN.  x fp32 [N, ldx]; rows int32, the list (NULL: list
 *   entry r is row r), seg_off int32 [n_seg + 1]; both are device data: a row index is clamped to [0, N - 1], an offset to
 *   [0, seg_off[n_seg]] and to its predecessor.  E % 4 == 0, ldx >= E and ldx % 4 == 0, x and out 16-byte aligned.  A
 *   protein's vector is a function of its own rows in list order, and the engine's rows are the same bits alone, padded and
 *   token-packed: an index does not depend on how it was batched.
 * esmk_op_topk_merge: one block of a streaming top-k.  Per row q the candidates are (S[q][j], id_base + j) for j < n_cols,
 *   except a NaN value and the column with id_base + j == exclude[q] (exclude int32 [n_rows] or NULL), and, unless first != 0,
 *   the used slots (id >= 0) of the running list val fp32 / id int32 [n_rows, k], whose ids the caller keeps disjoint from the
 *   block's.  The list receives the k best under value descending, then id ascending; values compare in the total order of
 *   their IEEE bits (-0.0 below +0.0; -inf is a value like any other); unused slots hold (-inf, -1) and stand behind every real
 *   candidate.  Columns at or behind n_cols are never candidates (the float4 group that holds column n_cols - 1 is loaded
 *   whole: ldS % 4 == 0).  first != 0 reads nothing of the lists.  One workgroup per row, one read of the row.
 *   Refused: null S or lists, k outside 1 .. 1024, n_cols outside 1 .. 2^22, ldS < n_cols or ldS % 4, id_base < 0 or
 *   id_base + n_cols > 2^31 - 1, S not 16-byte aligned, n_rows outside 0 .. 2^24 (0: nothing is launched). */
int esmk_op_pool_rows(const float* x_dev, int ldx, int N, const int32_t* rows_dev, const int32_t* seg_off_dev, int n_seg,
                      float* out_dev, int E, void* stream);
int esmk_op_topk_merge(const float* S_dev, int ldS, int n_rows, int n_cols, int id_base, const int32_t* exclude_dev, int k,
                       float* val_dev, int32_t* id_dev, int first, void* stream);

/* Range search and greedy incremental clustering on pooled embeddings (csrc/cluster.hip; esm_amd/cluster.py).  The
 * similarities are the same GEMM blocks as the search's.  No entry uses a float atomic or scratch memory; all results are the
 * same bits run after run.  Every entry checks its arguments before the first HIP call.
 * esmk_op_range_rows: one block of a thresholded row scan.  Column j < n_cols of row q passes when S[q][j] >= threshold as a
 *   float comparison (NaN never passes, a tie does, -0.0 >= +0.0 does; a NaN threshold passes nothing) and
 *   id_base + j != exclude[q] (exclude int32 [n_rows] or NULL).  Columns at or behind n_cols never pass (the float4 group
 *   that holds column n_cols - 1 is loaded whole: ldS % 4 == 0).  One workgroup per row, one read of the row.
 *   fill == 0, the count pass: counts[q] (int64 [n_rows]) += the number of passing columns of row q.
 *   fill != 0, the fill pass: the passing (id_base + j, S[q][j]) of row q, in ascending j, are written to ids / scores
 *   (int32 / fp32 [cap]) from position cursor[q] on, and cursor[q] (int64 [n_rows]) advances by their number: blocks given in
 *   ascending id_base leave row q's ids ascending.  Row q owns the positions offsets[q] .. offsets[q + 1] - 1 (offsets int64
 *   [n_rows + 1]).  offsets and cursor are device data: the range is clamped into [0, cap], its end to no less than
 *   its start, and the cursor into the range; a pair whose position is at or behind the range's end is not
 *   written, and the cursor never passes the end.
 *   Refused: null S; null counts (count pass); null offsets, cursor, ids or scores (fill pass); n_cols outside 1 .. 2^22;
 *   ldS < n_cols or ldS % 4; id_base < 0 or id_base + n_cols > 2^31 - 1; cap < 0; S not 16-byte aligned, counts / offsets /
 *   cursor not 8-byte aligned; n_rows outside 0 .. 2^24 (0: nothing is launched).
 * The graph entries read a CSR of out-lists: offsets int64 [n + 1], ids int32 [nnz] (device data: a list's range is clamped
 *   into [0, nnz], an id outside [0, n) is skipped), rank int32 [n] (a permutation of 0 .. n - 1: the lower rank is decided
 *   first) and state int32 [n]: 0 undecided, 1 a new representative (its out-list not yet covered), 2 a representative, 3
 *   covered.  lanes (a power of two, 1 .. 64) consecutive lanes walk one out-list.
 * esmk_op_cluster_mark: for every w of out-list u with rank[w] > rank[u]: blocked[w] = 1 if state[u] == 0, covered[w] = 1 if
 *   state[u] == 1 (int32 [n] each; plain stores of 1).  Reads state, writes only blocked and covered.
 * esmk_op_cluster_decide: per node u: state 1 -> 2; state 0 -> 3 if covered[u], else -> 1 unless blocked[u]; blocked[u] = 0;
 *   *remaining (int32, device) += the nodes still in state 0 (an integer atomic add per workgroup).
 *   A round is mark, then decide, from state = blocked = covered = 0; when *remaining of a round is 0 the states are those
 *   of the sequential greedy loop (walk by rank; an uncovered node becomes a representative and covers its out-list).
 * esmk_op_cluster_assign: key[w] (uint64 [n], zeroed by the caller) = the maximum over the representatives u (state 1 or 2)
 *   with w in out-list u and rank[u] < rank[w] of [o << 32 | 0xFFFFFFFF - rank[u]], o = 0 (nearest == 0: the representative
 *   of the lowest rank) or the order of scores[i] (fp32 [nnz]; nearest != 0: the largest score in the total order of the
 *   IEEE bits as in esmk_op_topk_merge, ties to the lower rank).  A 64-bit integer atomic max.
 *   Refused by all three: null offsets, rank, state or flag / key arrays, null ids with nnz > 0, n outside 1 .. 2^24,
 *   nnz < 0, lanes not a power of two in 1 .. 64, misaligned arrays. */
int esmk_op_range_rows(const float* S_dev, int ldS, int n_rows, int n_cols, int id_base, const int32_t* exclude_dev, float threshold,
                       int fill, int64_t* counts_dev, const int64_t* offsets_dev, int64_t* cursor_dev, int32_t* ids_dev,
                       float* scores_dev, long long cap, void* stream);
int esmk_op_cluster_mark(const int64_t* offsets_dev, const int32_t* ids_dev, int n, long long nnz, const int32_t* rank_dev,
                         const int32_t* state_dev, int32_t* blocked_dev, int32_t* covered_dev, int lanes, void* stream);
int esmk_op_cluster_decide(int32_t* state_dev, int32_t* blocked_dev, const int32_t* covered_dev, int n, int32_t* remaining_dev,
                           void* stream);
int esmk_op_cluster_assign(const int64_t* offsets_dev, const int32_t* ids_dev, const float* scores_dev, int n, long long nnz,
                           const int32_t* rank_dev, const int32_t* state_dev, int nearest, uint64_t* key_dev, int lanes, void* stream);

/* From search hits to a query-anchored MSA (csrc/msa_build.hip; esm_amd/msa_build.py).  Integer and comparison logic, no atomics,
 * no scratch memory; all results are the same bits whatever the launch geometry.  Both entries check their arguments before
 * the first HIP call.
 * esmk_op_msa_project: the alignment paths of the P hits of one query as rows of a byte matrix.  cols int32 [n_cols_total, 2]
 *   and col_offsets int64 [P + 1] as esmk_op_align_traceback leaves them (hit p owns cols[col_offsets[p] .. col_offsets[p + 1]);
 *   the offsets index from cols_dev, so a query's slice of a longer table is given by its col_offsets alone); seqs uint8
 *   [n_bytes], the hits' residues as one blob, hit p at seq_off[p] (int64 [P]) with seq_len[p] (int32 [P]) bytes; query uint8
 *   [Lq].  msa uint8 [P, ld]: columns 0 .. Lq - 1 of row p are '-' except msa[p][i] = seqs[seq_off[p] + j] for every path column
 *   (i, j) that is a match; columns Lq .. ld - 1 are 0.  A path column is a match when 0 <= i < Lq and 0 <= j < len, a deletion
 *   when 0 <= i < Lq and j == -1, an insertion when i == -1 and 0 <= j < len; any other column is ignored.  Everything is device
 *   data: len is seq_len[p] clamped to the bytes the blob holds behind seq_off[p] (0 for a seq_off outside the blob), the
 *   path's range is clamped into [0, n_cols_total] and its end to no less than its start.  stats int32 [P, 6]: n_match; n_ident
 *   (matches whose letter equals query[i]); n_ins and n_del, the insertions and deletions whose path position lies strictly
 *   between those of the first and the last match; the query columns of the first and of the last match (by path position;
 *   -1, -1 without a match).  A path that names a query column twice leaves one of its letters there.  One wavefront per hit.
 *   Refused: null col_offsets, seq_off, seq_len, query, msa or stats; null cols with n_cols_total > 0, null seqs with
 *   n_bytes > 0; negative n_cols_total or n_bytes; P outside 0 .. 2^24 (0: nothing is launched); Lq outside 1 .. 8192; ld < Lq
 *   or ld % 4; P * ld >= 2^31; col_offsets / seq_off not 8-byte aligned, cols / seq_len / msa / stats not 4-byte aligned.
 * esmk_op_msa_pair_identity: rows i0 .. i0 + nb - 1 of the gap-aware identity matrix of msa uint8 [N, ld] over the columns
 *   c < L.  both(r, j) = the columns in which neither row holds the gap byte, same(r, j) = those of them in which the bytes
 *   are equal; S[r - i0][j] = float(same) / float(both), one correctly rounded fp32 division, when both >= min_overlap, else
 *   0: never NaN.  S fp32 [nb, ldS]; columns N .. ldS - 1 are written as 0: a block is what esmk_op_range_rows takes.  Every
 *   byte value is legal, nothing at or behind column L is compared.  64 x 64 tiles, a workgroup owns its tile of S.
 *   Refused: null msa or S; N outside 1 .. 2^22; L outside 1 .. 65535; ld < L; N * ld >= 2^31; gap outside 0 .. 255;
 *   min_overlap < 1; a row block outside [0, N) or of more than 2^21 rows (nb == 0: nothing is launched); ldS < N, ldS % 4
 *   or ldS > 2^22; S not 16-byte aligned. */
int esmk_op_msa_project(const int32_t* cols_dev, long long n_cols_total, const int64_t* col_offsets_dev, int P, const uint8_t* seqs_dev,
                        long long n_bytes, const int64_t* seq_off_dev, const int32_t* seq_len_dev, const uint8_t* query_dev, int Lq,
                        uint8_t* msa_dev, int ld, int32_t* stats_dev, void* stream);
int esmk_op_msa_pair_identity(const uint8_t* msa_dev, int N, int L, int ld, int gap, int min_overlap, int i0, int nb, float* S_dev,
                              int ldS, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ESMK_H */
