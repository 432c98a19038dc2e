"""ctypes binding of libesmk.so (C ABI declared in include/esmk.h).

PyTorch is used only as the owner of device memory and streams: every call below takes raw
device pointers (``tensor.data_ptr()``) and the current HIP stream.  There is no CPU fallback:
if the shared library is missing or cannot be loaded the import of this module raises.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libesmk.so")

F32, F16, BF16 = 0, 1, 2
OUT_LOGITS, OUT_ATTN, OUT_CONTACTS, OUT_COL_ATTN, OUT_REPR_LOWP, OUT_ATTN_LOWP = 1, 2, 4, 8, 16, 32
EPI_STORE_T, EPI_STORE_F32, EPI_GELU_T, EPI_GELU_F32, EPI_RESID_F32 = 0, 1, 2, 3, 4
EPI_QKV_ROPE, EPI_V_T, EPI_MSA_CTX = 5, 6, 7
ESM1, ESM1_FINAL_BIAS = 2, 4  # esmk_config.no_rope values of the original ESM-1 architecture (include/esmk.h)
EDIT_AXPBY, EDIT_PROJECT, MAX_STREAM_EDITS = 0, 1, 64  # esmk_stream_edit.op; the longest list esmk_set_stream_edits takes


class EsmkConfig(ctypes.Structure):
    _fields_ = [
        ("num_layers", c_int32),
        ("embed_dim", c_int32),
        ("num_heads", c_int32),
        ("ffn_dim", c_int32),
        ("vocab", c_int32),
        ("pad_idx", c_int32),
        ("mask_idx", c_int32),
        ("cls_idx", c_int32),
        ("eos_idx", c_int32),
        ("token_dropout", c_int32),
        ("prepend_bos", c_int32),
        ("append_eos", c_int32),
        ("operand_dtype", c_int32),
        ("no_rope", c_int32),
        ("num_positions", c_int32),
        ("ln_before", c_int32),
        ("weight_split", c_int32),
        ("ln_fold", c_int32),
    ]


class EsmkMsaConfig(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in (
        "num_layers", "embed_dim", "num_heads", "ffn_dim", "vocab", "pad_idx", "mask_idx", "cls_idx", "eos_idx",
        "prepend_bos", "append_eos", "num_positions", "has_msa_position_embedding", "operand_dtype", "weight_split")]


class EsmkStreamEdit(ctypes.Structure):
    """esmk_stream_edit (include/esmk.h): one edit of the residual stream after ``layer`` layers."""
    _fields_ = [("layer", c_int32), ("op", c_int32), ("keep", c_float), ("gain", c_float),
                ("rows_dev", c_void_p), ("n_rows", c_int32), ("token_set", ctypes.c_uint64),
                ("src_dev", c_void_p), ("src_ld", c_int32), ("n_src", c_int32), ("src_index_dev", c_void_p)]


class EsmkProfileEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", c_int32), ("ms", ctypes.c_double),
                ("flops", ctypes.c_double), ("bytes", ctypes.c_double)]


class EsmkGemmExArgs(ctypes.Structure):
    """esmk_gemm_ex_args (include/esmk.h): one field per generalised GemmArgs field of the engine."""
    _fields_ = [
        ("size", c_size_t),
        ("A", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("out", c_void_p),
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("a_kt_repeat", c_int32),
        ("a_row_bytes", c_int64), ("w_row_bytes", c_int64), ("a_kt_bytes", c_int64), ("w_kt_bytes", c_int64),
        ("batch", c_int32), ("batch_inner", c_int32),
        ("a_bo", c_int64), ("a_bi", c_int64), ("w_bo", c_int64), ("w_bi", c_int64), ("o_bo", c_int64), ("o_bi", c_int64),
        ("n_valid", c_int32), ("ldc", c_int32),
        ("q", c_void_p), ("k", c_void_p), ("vt", c_void_p), ("cos", c_void_p), ("sin", c_void_p),
        ("T", c_int32), ("H", c_int32), ("E", c_int32), ("Tp", c_int32),
        ("scaling", c_float), ("vt_rows", c_int32),
        ("row_keep", c_void_p),
        ("rowmap_R", c_int32), ("rowmap_C", c_int32), ("ctx_R", c_int32), ("ctx_C", c_int32),
        ("head_dim", c_int32), ("epilogue", c_int32),
        ("row_pos", c_void_p),
        ("operand_dtype", c_int32), ("reserved", c_int32),
    ]


# name -> (restype, argtypes); must list every symbol include/esmk.h declares
SIGNATURES = {
    "esmk_last_error": (c_char_p, []),
    "esmk_version": (c_char_p, []),
    "esmk_create": (c_int, [POINTER(EsmkConfig), POINTER(c_void_p)]),
    "esmk_destroy": (None, [c_void_p]),
    "esmk_set_rope_inv_freq": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "esmk_packed_bytes": (c_int, [c_void_p, POINTER(c_size_t)]),
    "esmk_pack_weight": (
        c_int,
        [c_void_p, c_void_p, c_size_t, c_char_p, c_void_p, c_int, POINTER(c_int64), c_int, c_void_p],
    ),
    "esmk_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_uint32, POINTER(c_size_t)]),
    "esmk_forward": (
        c_int,
        [
            c_void_p, c_void_p, c_void_p, c_int, c_int,
            POINTER(c_int32), c_int, POINTER(c_void_p),
            c_uint32, c_void_p, c_void_p, c_void_p,
            c_void_p, c_size_t, c_void_p,
        ],
    ),
    "esmk_rows_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "esmk_forward_rows": (
        c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # design: selected log-prob rows and contact maps with the head-group count of B = 1 in one forward
    "esmk_rows_contacts_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "esmk_forward_rows_contacts": (
        c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "esmk_debug_contact_groups": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int32)]),
    # linear pairwise heads on the attention maps: the handle's head (host arrays), the row-selected forward with its output,
    # the kernels on stacked operands, the distogram cross-entropy
    "esmk_set_pair_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int]),
    "esmk_rows_pair_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "esmk_forward_rows_pair": (
        c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "esmk_op_pair_head_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "esmk_op_pair_head": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t,
                c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_distogram_energy": (
        c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    # sparse-autoencoder features of the stream (csrc/sae.hip): the operand image, the row-wise top-k, the per-sequence
    # maximum, the decode
    "esmk_op_sae_cand": (c_int, []),
    "esmk_op_sae_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_sae_topk": (c_int, [c_void_p, c_int, c_void_p, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "esmk_op_sae_segment_max": (c_int, [c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "esmk_op_sae_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    # embedding-based alignment (csrc/align.hip): the two operand images, the z-score enhancement, the affine-gap DP, the walk
    "esmk_op_align_panel": (c_int, []),
    "esmk_op_align_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_align_enhance": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "esmk_op_align_dp": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_void_p,
                                 c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "esmk_op_align_traceback": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "esmk_op_align_dp_ex": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_float, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "esmk_op_align_traceback_ex": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    # protein search on pooled embeddings (csrc/search.hip): the per-protein mean, the streaming top-k
    "esmk_op_pool_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "esmk_op_topk_merge": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    # range search and greedy clustering (csrc/cluster.hip): the thresholded row scan (count / fill), the rounds, the assignment
    "esmk_op_range_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int64, c_void_p]),
    "esmk_op_cluster_mark": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "esmk_op_cluster_decide": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "esmk_op_cluster_assign": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                       c_void_p]),
    # search hits to an MSA (csrc/msa_build.hip): alignment paths to rows of a byte matrix, gap-aware pairwise identity
    "esmk_op_msa_project": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p, c_int, c_void_p, c_void_p]),
    "esmk_op_msa_pair_identity": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    # early exit: the handle's layer limit
    "esmk_set_layer_limit": (c_int, [c_void_p, c_int]),
    # edits of the residual stream between layers: the handle's list, and one edit as a single op
    "esmk_set_stream_edits": (c_int, [c_void_p, POINTER(EsmkStreamEdit), c_int]),
    "esmk_op_stream_edit": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(EsmkStreamEdit), c_void_p, c_int, c_void_p, c_void_p,
                                    c_int, c_void_p]),
    # token-packed batch + row selection (mixed-length libraries of masked copies); the segment table is a host array
    "esmk_packed_rows_workspace_bytes": (
        c_int, [c_void_p, POINTER(c_int32), c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "esmk_forward_packed_rows": (
        c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                c_void_p]),
    "esmk_packed_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_uint32, POINTER(c_size_t)]),
    "esmk_forward_packed": (
        c_int,
        [
            c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int,
            POINTER(c_int32), c_int, POINTER(c_void_p),
            c_uint32, c_void_p, c_void_p, c_size_t, c_void_p,
        ],
    ),
    "esmk_packed_workspace_bytes_ex": (c_int, [c_void_p, POINTER(c_int32), c_int, c_int, c_uint32, POINTER(c_size_t)]),
    "esmk_forward_packed_ex": (
        c_int,
        [
            c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int,
            POINTER(c_int32), c_int, POINTER(c_void_p),
            c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
        ],
    ),
    "esmk_packed_workspace_bytes_maps": (c_int, [c_void_p, POINTER(c_int32), c_int, c_int, c_uint32, POINTER(c_size_t)]),
    "esmk_forward_packed_maps": (
        c_int,
        [
            c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int,
            POINTER(c_int32), c_int, POINTER(c_void_p),
            c_uint32, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p,
        ],
    ),
    "esmk_msa_create": (c_int, [POINTER(EsmkMsaConfig), POINTER(c_void_p)]),
    "esmk_msa_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, c_uint32, POINTER(c_size_t)]),
    "esmk_msa_forward": (
        c_int,
        [
            c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
            POINTER(c_int32), c_int, POINTER(c_void_p),
            c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
            c_void_p, c_size_t, c_void_p,
        ],
    ),
    "esmk_msa_rows_workspace_bytes": (
        c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    "esmk_msa_forward_rows": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "esmk_debug_msa_row_slices": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "esmk_profile_begin": (c_int, [c_void_p]),
    "esmk_profile_end": (c_int, [c_void_p, POINTER(EsmkProfileEntry), c_int, POINTER(c_int)]),
    "esmk_ln_fold_enabled": (c_int, [c_void_p]),
    "esmk_op_layernorm": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_masked_row_mean": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_linear": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    ),
    "esmk_debug_gemm_timing": (c_int, [c_void_p]),
    "esmk_debug_gemm_impl": (c_int, [c_int, c_int]),
    "esmk_debug_gemm_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int32)]),
    "esmk_debug_set": (c_int, [c_char_p, c_double]),
    "esmk_op_rowstats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_ln_finalize": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_fold_weight": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_fold_weight_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "esmk_op_linear_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "esmk_op_qkv_rope_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_void_p]),
    "esmk_debug_mma_selftest": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "esmk_op_split_weight": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_linear_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_linear_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_layernorm_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
                                     c_int, c_int, c_int, c_float, c_void_p]),
    "esmk_op_split_weight_ex": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    "esmk_op_linear_gelu_x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_debug_linear_splitk": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_qkv_rope": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    ),
    "esmk_op_qkv_rope2": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    ),
    "esmk_op_attention": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
         c_void_p],
    ),
    "esmk_op_attention_probs": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
         c_void_p],
    ),
    "esmk_op_attention_ex": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
         c_int, c_int, c_int, c_void_p],
    ),
    "esmk_op_attention_biaskv": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
         c_int, c_int, c_void_p],
    ),
    "esmk_op_attention_probs_ex": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
         c_int, c_int, c_void_p],
    ),
    "esmk_op_attention_packed": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    "esmk_op_attention_probs_packed": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
         c_void_p, c_size_t, c_void_p],
    ),
    "esmk_op_contacts_fused_workspace_bytes_ex": (
        c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "esmk_op_contacts_fused_ex": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_int, c_void_p,
         c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int),
         c_int, c_void_p],
    ),
    "esmk_op_gemm_ex": (c_int, [POINTER(EsmkGemmExArgs), c_void_p]),
    "esmk_op_msa_row_softmax": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
         c_void_p],
    ),
    "esmk_op_mask_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_log_softmax_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    # multi-mutant variants: a list of masked positions per copy; fp64 sums of fp32 log p(mt) - log p(wt) per variant
    "esmk_op_mask_rows_multi": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_score_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    # packed masked copies (esmk_forward_packed_rows' input); fp64 sums of the fp32 log p(true token) per sequence
    "esmk_op_mask_rows_packed": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                c_int, c_void_p]),
    "esmk_op_sum_target_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    # windows: window copies of long sequences, the owner / blend stitch of per-window rows, the stitch of per-window contact maps
    "esmk_op_window_rows": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                c_void_p]),
    "esmk_op_blend_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_stitch_contacts": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    # sampling: per-chain shuffles, one token per row of log-probabilities, the write-back (seeds and masks are uint64)
    "esmk_op_permute_positions": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_uint64, c_int, c_void_p]),
    "esmk_op_sample_rows": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint64, c_float, ctypes.c_uint64, c_int, c_void_p, c_void_p,
                c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_commit_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    # decoding: the draw behind a top-k / nucleus filter with a per-row confidence; the per-chain choice of the best rows
    "esmk_op_sample_rows_ex": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint64, c_float, ctypes.c_uint64, c_int, c_int, c_float, c_int,
                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_select_rows": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    # Metropolis-Hastings design: the proposal, the contact term of the energy, the acceptance, the LM proposal's correction
    "esmk_op_propose_mutations": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint64, c_int, ctypes.c_uint64, c_int, c_void_p,
                c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_contact_energy": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_mh_accept": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double,
                c_double, ctypes.c_uint64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                c_void_p]),
    "esmk_op_hastings_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]),
    # the n-gram term of the design energy, the acceptance with per-chain temperatures and a third term, the replica swap
    "esmk_op_ngram_energy": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                c_int, c_void_p]),
    "esmk_op_mh_accept_ex": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                c_double, c_double, c_void_p, c_void_p, c_int, ctypes.c_uint64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_replica_swap": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint64, c_int, c_void_p, c_void_p, c_int, c_int,
                c_void_p]),
    # MSA row selection: mismatch rows, neighbour counts, the greedy pick, race keys and their ranks (msa uint8 [N, ld])
    "esmk_op_msa_mismatch_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "esmk_op_msa_neighbor_counts": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "esmk_op_msa_greedy_select": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "esmk_op_msa_race_keys": (c_int, [c_void_p, c_int, ctypes.c_uint64, c_int, c_void_p, c_void_p]),
    "esmk_op_rank_keys": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    # the categorical Jacobian: substituted copies, the scatter of logit differences into J, centring, contact map, APC
    "esmk_op_substitute_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_jacobian_scatter": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_jacobian_center": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_jacobian_contacts": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_apc": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    # the token front end, one launch at a time (tests/test_frontend_ops_gpu.py); segment tables are host arrays
    "esmk_op_seq_stats": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "esmk_op_packed_stats": (
        c_int, [c_void_p, POINTER(c_int32), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                c_void_p]),
    "esmk_op_zero_gap_rows": (c_int, [c_void_p, POINTER(c_int32), c_int, c_int, c_size_t, c_void_p]),
    "esmk_op_embed": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "esmk_op_embed_esm1": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                c_void_p]),
    "esmk_op_add_positions": (
        c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int, c_int, c_void_p]),
    "esmk_op_scale_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_msa_embed": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                c_int, c_int, c_int, c_void_p]),
    "esmk_op_sinus_table": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_rope_table": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "esmk_op_gather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "esmk_op_contacts": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
         c_int, c_int, c_void_p],
    ),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m esm_amd.build` "
            "(needs hipcc; there is no CPU fallback for the engine)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class EsmkError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise EsmkError(lib.esmk_last_error().decode())


def dtype_code(torch_dtype):
    import torch

    return {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}[torch_dtype]


def torch_dtype(code):
    import torch

    return {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[code]


def cur_stream():
    import torch

    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)
