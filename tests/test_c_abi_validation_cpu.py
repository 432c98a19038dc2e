"""Argument validation of the C ABI (include/esmk.h) without a GPU: every check below fails BEFORE the library touches
the HIP runtime (dimension checks, missing output buffers for the requested flags, workspace size, the row limit, the
segment table of esmk_forward_packed), so the error codes and messages are testable in the build container.  Buffers
are fake non-null addresses: a call that got past validation would dereference nothing on the host either — it would
fail in hipMalloc / the first launch — but none of these calls gets that far."""
import ctypes

import pytest
import torch

from esm_amd import _native as N

FAKE = ctypes.c_void_p(0x1000)


def make(L=2, E=128, H=2, **kw):
    cfg = N.EsmkConfig(L, E, H, 4 * E, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


def err():
    return N.lib.esmk_last_error().decode()


def test_create_rejects_bad_dimensions():
    for kw, msg in ((dict(num_layers=0), "non-positive"), (dict(num_heads=3), "divisible"),
                    (dict(embed_dim=144, num_heads=1), "head_dim"),          # head_dim 144: not 128, not <= 64
                    (dict(operand_dtype=0), "operand_dtype"), (dict(ffn_dim=100), "multiple")):
        rc, _ = make(**kw)
        assert rc != 0 and msg in err(), (kw, err())
    rc, h = make()
    assert rc == 0
    N.lib.esmk_destroy(h)
    N.lib.esmk_destroy(None)  # like free(NULL)


def test_workspace_queries_and_row_limit():
    rc, h = make()
    n = ctypes.c_size_t()
    assert N.lib.esmk_workspace_bytes(h, 2, 64, N.OUT_LOGITS, ctypes.byref(n)) == 0
    base = n.value
    assert N.lib.esmk_workspace_bytes(h, 2, 64, N.OUT_LOGITS | N.OUT_ATTN | N.OUT_CONTACTS, ctypes.byref(n)) == 0
    materialised = n.value
    assert N.lib.esmk_workspace_bytes(h, 2, 64, N.OUT_CONTACTS, ctypes.byref(n)) == 0
    fused = n.value  # [T,T] accumulators + per-channel sums instead of the [L,H,T,T] scratch of the caller's tensor
    assert base < materialised and base < fused
    assert N.lib.esmk_workspace_bytes(h, 0, 64, N.OUT_LOGITS, ctypes.byref(n)) != 0 and "positive" in err()
    assert N.lib.esmk_workspace_bytes(h, 1 << 14, 1 << 11, N.OUT_LOGITS, ctypes.byref(n)) != 0 and "2^24" in err()
    assert N.lib.esmk_packed_workspace_bytes(h, 2, 100, N.OUT_LOGITS, ctypes.byref(n)) != 0  # rows % 64
    assert N.lib.esmk_packed_workspace_bytes(h, 2, 128, N.OUT_ATTN, ctypes.byref(n)) != 0
    assert N.lib.esmk_packed_workspace_bytes(h, 2, 128, N.OUT_LOGITS | N.OUT_REPR_LOWP, ctypes.byref(n)) == 0
    N.lib.esmk_destroy(h)


# Byte counts of the packed-batch workspaces, recorded from the build in front of the split of the forward engine into stages:
# the int32 tables behind the workspace ([seg 2n][npad n][work 4 items][pad][contact tables][pad][map offsets u64 n]) have ONE
# layout function since then, and it must give what the three hand-written copies gave.  First table: three segments, an odd
# slot count in front of the contact tables and of the map offsets (both alignment slots in use); second: 40 short segments,
# tables of more than one 256-byte carving unit.
PACKED_SEGS_A = ([0, 5, 16, 130, 160, 64], 256)
PACKED_SEGS_B = ([v for s in range(40) for v in (16 * s, 9 + s % 8)], 640)
_CT, _AT, _LG = N.OUT_CONTACTS, N.OUT_ATTN, N.OUT_LOGITS
PACKED_WORKSPACE_BYTES = [
    ("esmk_packed_workspace_bytes", PACKED_SEGS_A, _LG, 531968),
    ("esmk_packed_workspace_bytes_ex", PACKED_SEGS_A, _LG, 531968),
    ("esmk_packed_workspace_bytes_ex", PACKED_SEGS_A, _LG | _CT, 720384),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_A, _LG, 531968),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_A, _LG | _AT, 534016),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_A, _AT | N.OUT_ATTN_LOWP, 534016),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_A, _LG | _CT | _AT, 720384),
    ("esmk_packed_workspace_bytes", PACKED_SEGS_B, _LG, 1332224),
    ("esmk_packed_workspace_bytes_ex", PACKED_SEGS_B, _LG | _CT, 1421568),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_B, _LG | _AT, 1337600),
    ("esmk_packed_workspace_bytes_maps", PACKED_SEGS_B, _LG | _CT | _AT, 1421824),
]


@pytest.mark.parametrize("entry,table,flags,expect", PACKED_WORKSPACE_BYTES)
def test_packed_workspace_bytes_are_those_of_the_parent_build(entry, table, flags, expect):
    rc, h = make()
    seg, rows = table
    arr = (ctypes.c_int32 * len(seg))(*seg)
    n = ctypes.c_size_t()
    if entry == "esmk_packed_workspace_bytes":
        rc = N.lib.esmk_packed_workspace_bytes(h, len(seg) // 2, rows, flags, ctypes.byref(n))
    else:
        rc = getattr(N.lib, entry)(h, arr, len(seg) // 2, rows, flags, ctypes.byref(n))
    assert rc == 0, err()
    assert n.value == expect
    N.lib.esmk_destroy(h)


def test_forward_argument_checks():
    rc, h = make()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)

    def call(flags, logits=FAKE, attn=None, contacts=None, ws_bytes=1 << 40, B=2, T=16, n_repr=1, lay=layers, out=outs,
             tokens=FAKE, packed=FAKE, ws=FAKE):
        return N.lib.esmk_forward(h, packed, tokens, B, T, lay, n_repr, out, flags, logits, attn, contacts, ws,
                                  ctypes.c_size_t(ws_bytes), None)

    assert call(N.OUT_LOGITS, tokens=None) != 0 and "null" in err()
    assert call(N.OUT_LOGITS, B=0) != 0 and "positive" in err()
    assert call(N.OUT_LOGITS, logits=None) != 0 and "logits buffer" in err()
    assert call(N.OUT_LOGITS | N.OUT_ATTN) != 0 and "attention buffer" in err()
    assert call(N.OUT_LOGITS | N.OUT_CONTACTS) != 0 and "contacts buffer" in err()
    assert call(N.OUT_LOGITS | N.OUT_ATTN | N.OUT_CONTACTS | N.OUT_ATTN_LOWP, attn=FAKE, contacts=FAKE) != 0 \
        and "ESMK_OUT_ATTN_LOWP" in err()
    bad_layer = (ctypes.c_int32 * 1)(3)  # L = 2
    assert call(N.OUT_LOGITS, lay=bad_layer) != 0 and "repr layer" in err()
    assert call(N.OUT_LOGITS, ws_bytes=16) != 0 and "workspace too small" in err()
    N.lib.esmk_destroy(h)


def test_packed_segment_table_checks():
    rc, h = make()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)

    def call(seg, rows=128, flags=N.OUT_LOGITS):
        arr = (ctypes.c_int32 * len(seg))(*seg)
        return N.lib.esmk_forward_packed(h, FAKE, FAKE, arr, len(seg) // 2, rows, layers, 1, outs, flags, FAKE, FAKE,
                                         ctypes.c_size_t(16), None)

    assert call([0, 20, 32, 5], rows=100) != 0 and "multiple of 64" in err()
    assert call([0, 0]) != 0 and "empty segment" in err()
    assert call([0, 20, 24, 5]) != 0 and "multiples of 16" in err()
    assert call([16, 20]) != 0 and "start at row 0" in err()
    assert call([0, 40, 32, 5]) != 0 and "disjoint" in err()
    assert call([0, 20, 112, 30]) != 0 and "past the last row" in err()
    assert call([0, 20, 32, 5], flags=N.OUT_LOGITS | N.OUT_CONTACTS) != 0 and "padded batches" in err()
    assert call([0, 20, 32, 5]) != 0 and "workspace too small" in err()  # a valid table reaches the size check
    N.lib.esmk_destroy(h)


def test_msa_flag_check():
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    h = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    n = ctypes.c_size_t()
    assert N.lib.esmk_msa_workspace_bytes(h, 1, 4, 16, N.OUT_LOGITS, ctypes.byref(n)) == 0 and n.value > 0
    N.lib.esmk_destroy(h)


def test_handle_kind_mix_up_is_rejected():
    """An MSA handle passed to the ESM-2 entry points (and the other way round) is refused before anything is
    indexed: esmk_forward on an MSA handle used to walk the empty ESM-2 layer table."""
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    n = ctypes.c_size_t()
    assert N.lib.esmk_workspace_bytes(hm, 2, 64, N.OUT_LOGITS, ctypes.byref(n)) != 0 and "MSA handle" in err()
    assert N.lib.esmk_packed_workspace_bytes(hm, 2, 128, N.OUT_LOGITS, ctypes.byref(n)) != 0 and "ESM-2 handle" in err()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)
    assert N.lib.esmk_forward(hm, FAKE, FAKE, 2, 16, layers, 1, outs, N.OUT_LOGITS, FAKE, None, None, FAKE,
                              ctypes.c_size_t(1 << 40), None) != 0 and "MSA handle" in err()
    N.lib.esmk_destroy(hm)
    rc, h = make()
    assert N.lib.esmk_msa_workspace_bytes(h, 1, 4, 16, N.OUT_LOGITS, ctypes.byref(n)) != 0 and "MSA model handle" in err()
    N.lib.esmk_destroy(h)


def test_documented_config_struct_matches_header_and_binding():
    """A stale document must fail CI (Weak-9): the `_Cfg` field list of INTEGRATION.md's ctypes snippet, the
    `esmk_config` members of include/esmk.h, the shipped reference-side stub and esm_amd._native.EsmkConfig are ONE list —
    a maintainer who copies the documented snippet must pass a struct of the size esmk_create reads."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    native = [n for n, _ in N.EsmkConfig._fields_]
    # include/esmk.h: the int32_t members of `typedef struct { ... } esmk_config;`
    hdr = open(os.path.join(root, "include", "esmk.h")).read()
    body = re.search(r"typedef struct[^{]*\{(.*?)\}\s*esmk_config\s*;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    header = []
    for decl in re.findall(r"int32_t\s+([^;]+);", body):
        header += [v.strip() for v in decl.split(",")]
    assert header == native, (header, native)
    # the names inside the `_Cfg` class of the python snippet
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    snippet = re.search(r"class _Cfg\(ctypes\.Structure\):.*?_fields_\s*=\s*\[.*?for n in \((.*?)\)\]", doc, re.S).group(1)
    documented = re.findall(r'"(\w+)"', snippet)
    assert documented == native, (documented, native)
    # ... and the constructor call of the snippet passes one value per field
    call = re.search(r"cfg = _Cfg\((.*?)\)\s*#", doc, re.S).group(1)
    depth, nargs = 0, 1
    for ch in call:
        depth += ch in "([" 
        depth -= ch in ")]"
        nargs += ch == "," and depth == 0
    assert nargs == len(native), (nargs, len(native))
    # the shipped reference-side stub
    stub = open(os.path.join(root, "examples", "reference_binding", "_esmk.py")).read()
    m = re.search(r"_fields_\s*=\s*\[(.*?)\]\s*\n", stub, re.S)
    assert re.findall(r'"(\w+)"', m.group(1)) == native
    assert ctypes.sizeof(N.EsmkConfig) == 4 * len(native) == 72


def test_ln_fold_validation_without_gpu():
    """esmk_config.ln_fold: refused together with weight_split and for head_dim 128; with the fold a q/k/v or fc1 weight
    packed before the layer's LayerNorm parameters fails before the library touches the device."""
    h = ctypes.c_void_p()
    f16 = N.dtype_code(torch.float16)
    cfg = N.EsmkConfig(1, 128, 2, 512, 33, 1, 32, 0, 2, 1, 1, 1, f16, 0, 0, 0, 1, 1)
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and "ln_fold" in err()
    cfg = N.EsmkConfig(1, 256, 2, 1024, 33, 1, 32, 0, 2, 1, 1, 1, f16, 0, 0, 0, 0, 1)  # head_dim 128
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and "ln_fold" in err()
    cfg = N.EsmkConfig(1, 128, 2, 512, 33, 1, 32, 0, 2, 1, 1, 1, f16, 0, 0, 0, 0, 1)
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        nb = ctypes.c_size_t()
        assert N.lib.esmk_packed_bytes(h, ctypes.byref(nb)) == 0
        shape = (ctypes.c_int64 * 2)(128, 128)
        for key in (b"layers.0.self_attn.q_proj.weight", b"layers.0.self_attn.v_proj.weight", b"layers.0.fc1.weight"):
            rc = N.lib.esmk_pack_weight(h, FAKE, nb.value, key, FAKE, 0, shape, 2, None)
            assert rc != 0 and "LayerNorm" in err(), key
    finally:
        N.lib.esmk_destroy(h)
    # the fold is off by request: the same keys are plain conversions (which would touch the device: not called here)
    cfg = N.EsmkConfig(1, 128, 2, 512, 33, 1, 32, 0, 2, 1, 1, 1, f16, 0, 0, 0, 0, -1)
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    N.lib.esmk_destroy(h)


def test_attention_ex_argument_checks():
    """esmk_op_attention_ex / esmk_op_attention_probs_ex: every invalid combination of head_dim, mode, dtype and tile
    padding is refused before a launch (the buffers are fake)."""
    f16, bf16 = N.dtype_code(torch.float16), N.dtype_code(torch.bfloat16)

    def fwd(head_dim=64, mode=0, dt=f16, B=2, H=2, T=100, Tp=128, bias=FAKE, seq=None, anyp=None, q=FAKE):
        return N.lib.esmk_op_attention_ex(q, FAKE, FAKE, bias, seq, anyp, FAKE, None, B, H, T, Tp, head_dim, mode, dt,
                                          None)

    assert fwd(q=None) != 0 and "null" in err()
    assert fwd(T=0) != 0 and "positive" in err()
    for Tp in (100, 96, 64):  # not a multiple of 64 / shorter than T
        assert fwd(Tp=Tp) != 0 and "Tp" in err(), Tp
    for hd in (32, 96, 256):
        assert fwd(head_dim=hd) != 0 and "head_dim" in err(), hd
    assert fwd(dt=N.F32) != 0 and "operand_dtype" in err()
    assert fwd(mode=3) != 0 and "mode" in err()
    assert fwd(head_dim=128, mode=1) != 0 and "head_dim 64" in err()
    assert fwd(head_dim=128, mode=2) != 0 and "head_dim 64" in err()
    assert fwd(mode=2, dt=bf16) != 0 and "fp16" in err()
    assert fwd(seq=FAKE, bias=None) != 0 and "seq_info" in err()
    assert fwd(mode=1, seq=FAKE) != 0 and "seq_info" in err()
    assert fwd(mode=0, anyp=FAKE) != 0 and "any_pad" in err()

    def probs(head_dim=64, msa_C=0, out=f16, dt=f16, B=4, layer=0, L=1, anyp=None):
        return N.lib.esmk_op_attention_probs_ex(FAKE, FAKE, FAKE, None, anyp, FAKE, B, 2, 100, head_dim, layer, L,
                                                msa_C, out, dt, None)

    assert probs(head_dim=96) != 0 and "head_dim" in err()
    assert probs(out=bf16) != 0 and "out_dtype" in err()
    assert probs(layer=1) != 0 and "layer" in err()
    assert probs(msa_C=3, out=N.F32) != 0 and "msa_C" in err()          # B = 4 columns of a batch of 4 / 3
    assert probs(msa_C=2, out=f16) != 0 and "fp32" in err()
    assert probs(msa_C=2, head_dim=128, out=N.F32) != 0 and "head_dim 64" in err()
    assert probs(anyp=FAKE, out=N.F32) != 0 and "any_pad" in err()


def test_contacts_fused_ex_argument_checks():
    """esmk_op_contacts_fused_ex / esmk_op_contacts_fused_workspace_bytes_ex: null pointers, head-group overrides out
    of range, head_dim-128 groups over 20 heads, bad dtypes and inconsistent segment tables are refused before a launch
    (the buffers are fake)."""
    f16 = N.dtype_code(torch.float16)

    def seg_arr(pairs):
        flat = [v for p in pairs for v in p]
        return (ctypes.c_int32 * max(len(flat), 1))(*flat), len(pairs)

    def run(q=FAKE, lse=FAKE, tok=FAKE, w=FAKE, out=FAKE, ws=FAKE, nbytes=1 << 40, B=2, H=4, T=100, L=2, hd=64, G=0,
            dt=f16, bos=1, eos=1, seg=None):
        sp, n = seg_arr(seg) if seg is not None else (None, 0)
        used = ctypes.c_int(-1)
        rc = N.lib.esmk_op_contacts_fused_ex(q, FAKE, lse, None, tok, w, None, sp, n, out, ws, nbytes, B, H, T, L, hd,
                                              1, 2, bos, eos, G, ctypes.byref(used), dt, None)
        assert rc == 0 or used.value == -1  # a refusal reports nothing
        return rc

    def size(B=2, H=4, T=100, L=2, hd=64, G=0, bos=1, eos=1, seg=None):
        sp, n = seg_arr(seg) if seg is not None else (None, 0)
        nb = ctypes.c_size_t()
        return N.lib.esmk_op_contacts_fused_workspace_bytes_ex(B, H, T, L, hd, sp, n, bos, eos, G, ctypes.byref(nb)), nb

    for kw in (dict(q=None), dict(lse=None), dict(tok=None), dict(w=None), dict(out=None), dict(ws=None)):
        assert run(**kw) != 0 and "null" in err(), kw
    assert N.lib.esmk_op_contacts_fused_workspace_bytes_ex(2, 4, 100, 2, 64, None, 0, 1, 1, 0, None) != 0
    assert "null" in err()
    for kw in (dict(B=0), dict(H=0), dict(T=0), dict(L=0)):
        assert run(**kw) != 0 and "positive" in err(), kw
    for hd in (32, 96, 256):
        assert run(hd=hd) != 0 and "head_dim" in err(), hd
    for dt in (N.F32, 7):
        assert run(dt=dt) != 0 and "operand_dtype" in err(), dt
    assert run(bos=2) != 0 and "prepend_bos" in err()
    assert run(T=2) != 0 and "no contact map" in err()  # S = T - 2 = 0
    for G in (-1, 5):  # H = 4
        assert run(G=G) != 0 and "head_groups" in err(), G
    assert run(hd=128, H=41, G=2) != 0 and "20 heads" in err()  # 21 heads per group
    assert run(hd=128, H=40, G=1) != 0 and "20 heads" in err()
    assert run(H=40, G=1, nbytes=0) != 0 and "workspace" in err()  # head_dim 64 takes 40 heads: past the checks
    rc, nb = size(hd=128, H=40, G=2)
    assert rc == 0 and nb.value > 0
    rc, nb = size(hd=128, H=40, G=1)
    assert rc != 0 and "20 heads" in err()
    # segment tables
    for seg, msg in (([(0, 100), (90, 20)], "overlap"), ([(200, 100)], "inside"), ([(-1, 10)], "inside"),
                     ([(0, -3)], "inside"), ([(10, 20), (0, 11)], "overlap")):
        assert run(B=1, T=256, seg=seg) != 0 and msg in err(), seg
        rc, _ = size(B=1, T=256, seg=seg)
        assert rc != 0 and msg in err(), seg
    assert run(B=2, T=256, seg=[(0, 10)]) != 0 and "B = 1" in err()
    sp, _ = seg_arr([(0, 10)])
    nb = ctypes.c_size_t()
    assert N.lib.esmk_op_contacts_fused_workspace_bytes_ex(1, 4, 256, 2, 64, sp, 0, 1, 1, 0, ctypes.byref(nb)) != 0
    assert "n_seg" in err()
    assert N.lib.esmk_op_contacts_fused_workspace_bytes_ex(1, 4, 256, 2, 64, None, 3, 1, 1, 0, ctypes.byref(nb)) != 0
    assert "n_seg" in err()
    # gaps, unsorted, a late first segment and empty segments are a valid table (sized, not run)
    rc, nb = size(B=1, T=512, seg=[(300, 130), (17, 2), (40, 0), (100, 129), (20, 1)])
    assert rc == 0 and nb.value > 0
    assert run(B=1, T=512, seg=[(300, 130), (17, 2)], nbytes=0) != 0 and "workspace" in err()


def gemm_args(**kw):
    """A valid tied-score launch of esmk_op_gemm_ex (engine_msa.hip: B = 1, S = 1, H = 2, R = 2, C = 100) on fake
    addresses, with the fields in `kw` replaced."""
    a = N.EsmkGemmExArgs()
    a.size = ctypes.sizeof(a)
    f = dict(A=0x1000, W=0x2000, out=0x3000, M=100, N=128, K=128, n_valid=100, ldc=128, a_row_bytes=128,
             w_row_bytes=128, a_kt_bytes=2 * 100 * 64 * 2, w_kt_bytes=2 * 100 * 64 * 2, batch=2, batch_inner=2,
             a_bi=100 * 64 * 2, w_bi=100 * 64 * 2, o_bi=100 * 128 * 4, head_dim=64, scaling=1.0,
             epilogue=N.EPI_STORE_F32, operand_dtype=N.F16)
    f.update(kw)
    for k, v in f.items():
        setattr(a, k, v)
    return a


def test_gemm_ex_argument_checks():
    assert ctypes.sizeof(N.EsmkGemmExArgs) == 264  # include/esmk.h: no padding between the fields
    call = lambda **kw: N.lib.esmk_op_gemm_ex(ctypes.byref(gemm_args(**kw)), None)  # noqa: E731
    assert N.lib.esmk_op_gemm_ex(None, None) != 0 and "null" in err()
    assert call(size=8) != 0 and "sizeof" in err()
    for kw in (dict(A=None), dict(W=None), dict(out=None)):
        assert call(**kw) != 0 and "null" in err(), kw
    for kw in (dict(epilogue=-1), dict(epilogue=8)):
        assert call(**kw) != 0 and "epilogue must be" in err(), kw
    for dt in (N.F32, 3):
        assert call(operand_dtype=dt) != 0 and "operand_dtype" in err(), dt
    for kw in (dict(M=0), dict(N=-8), dict(K=0)):
        assert call(**kw) != 0 and "positive" in err(), kw
    for kw in (dict(K=96), dict(N=100, n_valid=0, ldc=0)):
        assert call(**kw) != 0 and "K % 64" in err(), kw
    assert call(epilogue=N.EPI_MSA_CTX, N=136, ldc=0, n_valid=0) != 0 and "N % 64" in err()
    for hd in (0, 32, 96, 256):
        assert call(head_dim=hd) != 0 and "head_dim" in err(), hd
    assert call(head_dim=128) != 0 and "head_dim 128 belongs" in err()
    for kw in (dict(batch=0), dict(batch_inner=0), dict(batch=3, batch_inner=2)):
        assert call(**kw) != 0 and "batch_inner" in err(), kw
    for f in ("a_row_bytes", "w_kt_bytes", "a_bo", "o_bi", "n_valid", "ldc"):
        assert call(**{f: -1}) != 0 and "negative" in err(), f
    assert call(a_kt_repeat=2) != 0 and "a_kt_repeat" in err()
    assert call(a_kt_repeat=1, K=192) != 0 and "a_kt_repeat" in err()
    assert call(n_valid=129) != 0 and "n_valid" in err()
    assert call(ldc=120) != 0 and "ldc" in err()
    # fp32 gelu exists for dense calls only
    assert call(epilogue=N.EPI_GELU_F32) != 0 and "epilogue 3" in err()
    assert call(epilogue=N.EPI_GELU_F32, n_valid=0, ldc=0, a_row_bytes=0, w_row_bytes=0, a_kt_bytes=0, w_kt_bytes=0,
                batch=1, batch_inner=1, a_kt_repeat=1, K=256) != 0 and "epilogue 3" in err()
    # fields that belong to one epilogue
    assert call(row_keep=0x4000) != 0 and "row_keep" in err()
    assert call(row_pos=0x4000) != 0 and "row_pos" in err()
    assert call(vt_rows=2) != 0 and "vt_rows" in err()
    assert call(ctx_R=2, ctx_C=100) != 0 and "ctx_R" in err()
    assert call(rowmap_R=2, rowmap_C=50) != 0 and "row map" in err()
    dense = dict(n_valid=0, ldc=0, a_row_bytes=0, w_row_bytes=0, a_kt_bytes=0, w_kt_bytes=0, batch=1, batch_inner=1,
                 a_bi=0, w_bi=0, o_bi=0, M=600, N=768, K=768)
    for kw in (dict(rowmap_R=7, rowmap_C=0), dict(rowmap_R=7, rowmap_C=65)):  # 600 % 455 != 0
        assert call(epilogue=N.EPI_RESID_F32, **dense, **kw) != 0 and "row map" in err(), kw
    # q / k / v forms
    qk = dict(dense, epilogue=N.EPI_QKV_ROPE, out=None, q=0x5000, k=0x6000, cos=0x7000, sin=0x8000, T=100, H=12,
              E=768, N=1536)
    vt = dict(dense, epilogue=N.EPI_V_T, out=None, vt=0x5000, T=100, H=12, E=768, Tp=128)
    for f in ("q", "k", "cos", "sin"):
        assert call(**dict(qk, **{f: None})) != 0 and "needs q, k, cos and sin" in err(), f
    assert call(**dict(vt, vt=None)) != 0 and "needs vt" in err()
    for kw in (dict(T=0), dict(H=0), dict(E=640), dict(N=768), dict(T=7)):  # 600 % 7 != 0
        assert call(**dict(qk, **kw)) != 0 and "E = H head_dim" in err(), kw
    for kw in (dict(Tp=64), dict(Tp=120)):
        assert call(**dict(vt, **kw)) != 0 and "Tp" in err(), kw
    assert call(**dict(vt, vt_rows=4)) != 0 and "vt_rows must divide" in err()  # 6 sequences
    assert call(**dict(vt, vt_rows=2, head_dim=128, H=6)) != 0 and "vt_rows needs head_dim 64" in err()
    # the context form
    ctx = dict(dense, epilogue=N.EPI_MSA_CTX, M=100, N=7 * 64, K=128, ldc=768, batch=12, batch_inner=12, ctx_R=7,
               ctx_C=100)
    for kw in (dict(ctx_R=0), dict(ctx_C=99), dict(ctx_R=6), dict(ldc=704)):
        assert call(**dict(ctx, **kw)) != 0 and "epilogue 7 needs" in err(), kw


def test_msa_row_softmax_argument_checks():
    def call(scores=FAKE, keep=FAKE, any_pad=FAKE, probs=FAKE, attn=None, B=1, H=2, R=3, C=100, ldp=128, layer=0,
             Ltot=1, nslice=1, dt=N.F16):
        return N.lib.esmk_op_msa_row_softmax(scores, keep, any_pad, probs, attn, B, H, R, C, ldp, layer, Ltot, nslice,
                                             dt, None)

    for kw in (dict(scores=None), dict(keep=None), dict(any_pad=None), dict(probs=None)):
        assert call(**kw) != 0 and "null" in err(), kw
    for kw in (dict(B=0), dict(H=0), dict(R=0), dict(C=0)):
        assert call(**kw) != 0 and "positive" in err(), kw
    for kw in (dict(C=1025, ldp=1088), dict(C=100, ldp=1088), dict(C=100, ldp=64)):
        assert call(**kw) != 0 and "ldp" in err(), kw
    assert call(nslice=0) != 0 and "nslice" in err()
    for kw in (dict(layer=1, Ltot=1), dict(layer=-1, Ltot=2)):
        assert call(attn=FAKE, **kw) != 0 and "layer" in err(), kw
    for dt in (N.F32, 5):
        assert call(dt=dt) != 0 and "operand_dtype" in err(), dt


def test_linear_f32_argument_checks():
    """esmk_op_linear_f32 (gemm32.hip as a single op): every shape the kernel's 16-byte loads and its output stride do
    not cover is refused before a launch (the buffers are fake)."""
    def call(a=FAKE, w=FAKE, out=FAKE, M=5, N=33, K=64, lda=None, ldc=None, gelu=0):
        return N_.esmk_op_linear_f32(a, K if lda is None else lda, w, None, out, N if ldc is None else ldc, M, N, K, gelu,
                                     None)

    N_ = N.lib
    for kw in (dict(a=None), dict(w=None), dict(out=None)):
        assert call(**kw) != 0 and "esmk_op_linear_f32: null" in err(), kw
    for kw in (dict(M=0), dict(N=-1), dict(K=0)):
        assert call(**kw) != 0 and "esmk_op_linear_f32" in err() and "positive" in err(), kw
    for K in (16, 48, 100):
        assert call(K=K) != 0 and "esmk_op_linear_f32" in err() and "K % 32" in err(), K
    for lda in (66, 65, 32, 60):  # not a multiple of 4 / shorter than K
        assert call(lda=lda) != 0 and "esmk_op_linear_f32" in err() and "lda" in err(), lda
    assert call(ldc=32) != 0 and "esmk_op_linear_f32" in err() and "ldc" in err()


def test_layernorm_ex_argument_checks():
    """esmk_op_layernorm_ex: what the LayerNorm kernel's addressing does not cover — above all the hi | hi | lo rows of the
    f16x3 mode — is refused before a launch (the buffers are fake)."""
    f16, bf16 = N.dtype_code(torch.float16), N.dtype_code(torch.bfloat16)

    def call(x=FAKE, g=FAKE, b=FAKE, y=FAKE, y32=None, rows=30, E=320, dt=f16, keep=None, map_R=0, map_C=0, ldy=0, x3=0,
             eps=1e-5):
        return N.lib.esmk_op_layernorm_ex(x, g, b, y, y32, rows, E, dt, keep, map_R, map_C, ldy, x3, eps, None)

    who = "esmk_op_layernorm_ex"
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(y=None, y32=None)):
        assert call(**kw) != 0 and who + ": null" in err(), kw
    for kw in (dict(rows=0), dict(E=0)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
    for E in (322, 5124, 8192):  # E % 4 != 0; E > 5120
        assert call(E=E) != 0 and who in err() and "E % 4" in err(), E
    assert call(dt=N.F32) != 0 and who in err() and "operand_dtype" in err()
    x3 = dict(x3=1, ldy=960)
    for kw in (dict(x3, E=96, ldy=288), dict(x3, ldy=959 // 4 * 4), dict(x3, ldy=0), dict(x3, y=None, y32=FAKE),
               dict(x3, dt=bf16)):
        assert call(**kw) != 0 and who + ": x3" in err(), kw
    for ldy in (4, 316, -4, 322):  # inside (0, E); negative; no 8-byte stores
        assert call(ldy=ldy) != 0 and who in err() and "ldy" in err(), ldy
    for kw in (dict(map_R=4, map_C=5), dict(map_R=3, map_C=0), dict(map_R=-1, map_C=5), dict(map_R=3, map_C=7)):
        assert call(**kw) != 0 and who in err() and "row map" in err(), kw
    for eps in (0.0, -1e-5, float("nan")):
        assert call(eps=eps) != 0 and who in err() and "eps" in err(), eps


def test_fold_weight_ex_argument_checks():
    """esmk_op_fold_weight_ex: head_dim and whole heads are checked before a launch, after them the checks of
    esmk_op_fold_weight, which stays as it was for any N (the buffers are fake)."""
    f16 = N.dtype_code(torch.float16)

    def call(w=FAKE, gamma=FAKE, beta=FAKE, dst=FAKE, b2=FAKE, n=96, k=64, ld=64, d=16):
        return N.lib.esmk_op_fold_weight_ex(w, N.F32, gamma, beta, dst, f16, b2, n, k, ld, d, None)

    who = "esmk_op_fold_weight"
    for d in (0, -16, 8, 48, 65, 128):
        assert call(d=d) != 0 and who + "_ex: head_dim" in err(), d
    for kw in (dict(n=100, d=16), dict(n=96, d=64), dict(n=40, d=24), dict(n=16, d=32)):
        assert call(**kw) != 0 and who + "_ex" in err() and "whole heads" in err(), kw
    for kw in (dict(w=None), dict(gamma=None), dict(beta=None), dict(dst=None), dict(b2=None)):
        assert call(**kw) != 0 and who + ": null" in err(), kw
    for kw in (dict(n=0), dict(n=-16), dict(k=0), dict(ld=63)):
        assert call(**kw) != 0 and who in err() and "ld >= K" in err(), kw
    # the entry without head_dim: the same checks, no condition on N
    old = lambda **kw: N.lib.esmk_op_fold_weight(kw.get("w", FAKE), N.F32, FAKE, FAKE, FAKE, f16, FAKE, kw.get("n", 130), 64,
                                                 kw.get("ld", 64), None)
    assert old(w=None) != 0 and who + ": null" in err()
    assert old(n=0) != 0 and "ld >= K" in err()
    assert old(ld=32) != 0 and "ld >= K" in err()


def test_split_weight_ex_argument_checks():
    """esmk_op_split_weight_ex: parts, the head-spreading maps and the row stride of the image are checked before a launch
    (the buffers are fake)."""
    f16 = N.dtype_code(torch.float16)

    def call(w=FAKE, dst=FAKE, wdt=N.F32, ddt=f16, rows=48, cols=128, ld=128, parts=3, rmap=0, cmap=0, d=16):
        return N.lib.esmk_op_split_weight_ex(w, wdt, dst, ddt, rows, cols, ld, parts, rmap, cmap, d, None)

    who = "esmk_op_split_weight_ex"
    for kw in (dict(w=None), dict(dst=None)):
        assert call(**kw) != 0 and who + ": null" in err(), kw
    for kw in (dict(rows=0), dict(cols=-64)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
    for parts in (0, 4, -1):
        assert call(parts=parts) != 0 and who in err() and "parts must be" in err(), parts
    for kw in (dict(wdt=3), dict(ddt=7, parts=1)):
        assert call(**kw) != 0 and who in err() and "dtypes" in err(), kw
    for kw in (dict(parts=2, ddt=N.F32), dict(parts=3, ddt=N.dtype_code(torch.bfloat16))):
        assert call(**kw) != 0 and who in err() and "fp16" in err(), kw
    assert call(rmap=2) != 0 and who in err() and "row_map" in err()
    for d in (0, -16, 65, 96, 127, 256):
        assert call(rmap=1, d=d) != 0 and who in err() and "head_dim must be" in err(), d
    for kw in (dict(rmap=1, rows=50), dict(cmap=1, cols=72, ld=320), dict(rmap=1, d=128, rows=192)):
        assert call(**kw) != 0 and who in err() and "divide" in err(), kw
    for kw in (dict(ld=64), dict(cmap=1, cols=48, ld=128), dict(cmap=1, d=128, cols=256, ld=192), dict(parts=1, ld=127)):
        assert call(**kw) != 0 and who in err() and "dst_ld is smaller" in err(), kw  # 3 heads of 16 spread to 192
    for kw in (dict(parts=2, ld=160), dict(parts=3, cols=100, ld=100)):
        assert call(**kw) != 0 and who in err() and "dst_ld % 64" in err(), kw


def test_linear_gelu_x3_argument_checks():
    """esmk_op_linear_gelu_x3, and the kernel-level contract behind it: the hi | hi | lo store of a 64-column block would
    leave a row of 3 N columns when N % 64 != 0 (and the buffer, for the last row), so neither the entry nor gemm_plan
    takes such a call — the engine's ffn_dim % 64 == 0 rule is no longer the only guard."""
    def call(a=FAKE, w=FAKE, bias=FAKE, out=FAKE, M=300, N=256, K3=192):
        return N_.esmk_op_linear_gelu_x3(a, w, bias, out, M, N, K3, None)

    N_ = N.lib
    who = "esmk_op_linear_gelu_x3"
    for kw in (dict(a=None), dict(w=None), dict(bias=None), dict(out=None)):
        assert call(**kw) != 0 and who + ": null" in err(), kw
    for kw in (dict(M=0), dict(N=0), dict(K3=-192)):
        assert call(**kw) != 0 and who in err() and "positive" in err(), kw
    for K3 in (64, 128, 320, 200):
        assert call(K3=K3) != 0 and who in err() and "K3 % 192" in err(), K3
    for n in (264, 8, 100, 1288):
        assert call(N=n) != 0 and who in err() and "N % 64" in err(), n
    # the plan itself (flag 32 = the x3_out form): gemm9 or nothing
    out = (ctypes.c_int32 * 4)()
    assert N_.esmk_debug_gemm_plan(300, 256, 192, N.EPI_GELU_T, 32, out) == 0 and out[0] == 9 and out[1] == 0
    assert N_.esmk_debug_gemm_plan(300, 264, 192, N.EPI_GELU_T, 32, out) == 0 and out[0] == 0
    assert N_.esmk_debug_gemm_plan(300, 264, 192, N.EPI_GELU_T, 0, out) == 0 and out[0] == 9  # the plain form takes N % 8
    for epi, flags in ((N.EPI_STORE_T, 32), (N.EPI_GELU_T, 32 | 4), (N.EPI_GELU_T, 64)):
        assert N_.esmk_debug_gemm_plan(300, 256, 192, epi, flags, out) != 0 and "esmk_debug_gemm_plan" in err()


# ---- the token front end (esmk_op_seq_stats ... esmk_op_gather_rows): refused before any HIP call, on fake pointers ----------
def _segs(table):
    return (ctypes.c_int32 * len(table))(*table), len(table) // 2


BAD_SEGMENT_TABLES = [([0, 20, 32, 5], 100, "multiple of 64"), ([0, 0], 128, "empty segment"),
                      ([0, 20, 24, 5], 128, "multiples of 16"), ([16, 20], 128, "start at row 0"),
                      ([0, 40, 32, 5], 128, "disjoint"), ([32, 5, 0, 20], 128, "start at row 0"),
                      ([0, 20, 112, 30], 128, "past the last row"), ([], 128, "positive"), ([0, 20], 0, "positive")]


def test_frontend_stats_argument_checks():
    L = N.lib

    def stats(tok=FAKE, B=3, T=70, scale=FAKE, kb=FAKE, info=FAKE, keep=None):
        return L.esmk_op_seq_stats(tok, B, T, 1, 32, 1, scale, kb, info, keep, None)

    for kw in (dict(tok=None), dict(scale=None), dict(kb=None), dict(info=None)):
        assert stats(**kw) != 0 and "esmk_op_seq_stats: null" in err(), kw
    for kw in (dict(B=0), dict(T=0), dict(T=-3)):
        assert stats(**kw) != 0 and "esmk_op_seq_stats" in err() and "positive" in err(), kw
    assert stats(B=1 << 14, T=1 << 11) != 0 and "2^24" in err()

    def packed(table=PACKED_SEGS_A[0], rows=PACKED_SEGS_A[1], tok=FAKE, scale=FAKE, kb=FAKE, pos=FAKE, npad=FAKE, seg=True):
        arr, n = _segs(table)
        return L.esmk_op_packed_stats(tok, arr if seg else None, n, rows, 1, 32, scale, kb, pos, npad, None, None)

    for kw in (dict(tok=None), dict(scale=None), dict(kb=None), dict(pos=None), dict(npad=None)):
        assert packed(**kw) != 0 and "esmk_op_packed_stats: null argument" in err(), kw
    assert packed(seg=False) != 0 and "esmk_op_packed_stats: null segment table" in err()
    for table, rows, msg in BAD_SEGMENT_TABLES:
        assert packed(table=table, rows=rows) != 0 and "esmk_op_packed_stats" in err() and msg in err(), (table, err())

    def gaps(table=PACKED_SEGS_A[0], rows=PACKED_SEGS_A[1], buf=FAKE, row_bytes=640, seg=True):
        arr, n = _segs(table)
        return L.esmk_op_zero_gap_rows(buf, arr if seg else None, n, rows, ctypes.c_size_t(row_bytes), None)

    assert gaps(buf=None) != 0 and "esmk_op_zero_gap_rows: null argument" in err()
    assert gaps(seg=False) != 0 and "esmk_op_zero_gap_rows: null segment table" in err()
    for rb in (0, 8, 24, 636, 1 << 31):
        assert gaps(row_bytes=rb) != 0 and "esmk_op_zero_gap_rows: row_bytes" in err(), rb
    for table, rows, msg in BAD_SEGMENT_TABLES:
        assert gaps(table=table, rows=rows) != 0 and "esmk_op_zero_gap_rows" in err() and msg in err(), (table, err())


def test_frontend_embedding_argument_checks():
    L = N.lib

    def embed(tok=FAKE, table=FAKE, scale=FAKE, x=FAKE, B=2, T=9, E=96, vocab=33, dropout=1):
        return L.esmk_op_embed(tok, table, scale, x, B, T, E, vocab, 1, 32, dropout, None)

    def esm1(tok=FAKE, table=FAKE, scale=None, sinus=FAKE, x=FAKE, B=2, T=9, E=96, vocab=35, dropout=0):
        return L.esmk_op_embed_esm1(tok, table, scale, sinus, x, B, T, E, vocab, 1, 33, dropout, 9.8, None)

    for fn, who, nulls in ((embed, "esmk_op_embed", (dict(tok=None), dict(table=None), dict(x=None), dict(scale=None))),
                           (esm1, "esmk_op_embed_esm1", (dict(tok=None), dict(table=None), dict(x=None), dict(sinus=None),
                                                         dict(scale=None, dropout=1)))):
        for kw in nulls:
            assert fn(**kw) != 0 and who + ": null argument" in err(), (who, kw)
        for kw in (dict(B=0), dict(T=0), dict(vocab=0)):
            assert fn(**kw) != 0 and who + ":" in err() and "positive" in err(), (who, kw)
        for E in (0, -4, 2, 98, 321):
            assert fn(E=E) != 0 and who + ": E must be a positive multiple of 4" in err(), (who, E)
        assert fn(B=1 << 14, T=1 << 11) != 0 and who in err() and "2^24" in err()

    def addpos(tok=FAKE, pos=FAKE, x=FAKE, B=2, T=600, E=96, pad=1, npos=1026, table=None, rows=0, n_seg=None):
        arr, n = _segs(table) if table is not None else (None, 0)
        return L.esmk_op_add_positions(tok, pos, x, B, T, E, pad, npos, arr, n if n_seg is None else n_seg, rows, None)

    who = "esmk_op_add_positions"
    for kw in (dict(tok=None), dict(pos=None), dict(x=None)):
        assert addpos(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(B=0), dict(T=0)):
        assert addpos(**kw) != 0 and who in err() and "positive" in err(), kw
    for E in (0, 6, 98):
        assert addpos(E=E) != 0 and who + ": E must be a positive multiple of 4" in err(), E
    assert addpos(npos=0) != 0 and who + ": npos" in err()
    for T in (16381, 100000):  # (T + 4) * 4 > 65536
        assert addpos(T=T, npos=1 << 20) != 0 and who in err() and "dynamic LDS" in err(), T
    for kw in (dict(T=1025), dict(T=600, npos=601), dict(T=5, npos=8, pad=3)):  # T > npos - pad_idx - 1
        assert addpos(**kw) != 0 and who in err() and "above the maximum of the positional embedding" in err(), kw
    assert addpos(n_seg=2) != 0 and who in err() and "without a segment table" in err()
    assert addpos(rows=64) != 0 and who in err() and "without a segment table" in err()
    for table, rows, msg in BAD_SEGMENT_TABLES:
        assert addpos(table=table, rows=rows, B=len(table) // 2 or 1, T=40) != 0 and who in err() and msg in err(), (table, err())
    ok_table = [0, 300, 304, 7]
    for kw in (dict(B=3, T=300), dict(B=2, T=299)):  # B != n_seg; T below the longest segment
        assert addpos(table=ok_table, rows=320, **kw) != 0 and who in err() and "longest segment" in err(), kw
    assert addpos(table=ok_table, rows=320, B=2, T=300, npos=300) != 0 and "above the maximum" in err()

    def scale_rows(x=FAKE, keep=FAKE, rows=77, E=96):
        return L.esmk_op_scale_rows(x, keep, rows, E, None)

    for kw in (dict(x=None), dict(keep=None)):
        assert scale_rows(**kw) != 0 and "esmk_op_scale_rows: null argument" in err(), kw
    for rows in (0, -1, (1 << 24) + 1):
        assert scale_rows(rows=rows) != 0 and "esmk_op_scale_rows: rows" in err(), rows
    for E in (0, 6):
        assert scale_rows(E=E) != 0 and "esmk_op_scale_rows: E must be a positive multiple of 4" in err(), E

    def msa(tok=FAKE, te=FAKE, pe=FAKE, mp=None, x=FAKE, keep=FAKE, fill=FAKE, anyp=FAKE, B=1, R=3, C=130, D=96, vocab=33,
            pad=1, npos=1026):
        return L.esmk_op_msa_embed(tok, te, pe, mp, x, keep, fill, anyp, B, R, C, D, vocab, pad, npos, None)

    who = "esmk_op_msa_embed"
    for kw in (dict(tok=None), dict(te=None), dict(pe=None), dict(x=None), dict(keep=None), dict(fill=None), dict(anyp=None)):
        assert msa(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(B=0), dict(R=0), dict(C=0), dict(vocab=0)):
        assert msa(**kw) != 0 and who in err() and "positive" in err(), kw
    for D in (0, 6, 770):
        assert msa(D=D) != 0 and who + ": D must be a positive multiple of 4" in err(), D
    assert msa(C=16381, npos=1 << 20) != 0 and who in err() and "dynamic LDS" in err()
    for kw in (dict(C=1025), dict(C=130, npos=131)):
        assert msa(**kw) != 0 and who in err() and "above the maximum of the positional embedding" in err(), kw
    assert msa(B=1 << 8, R=1 << 8, C=1 << 9, npos=1 << 20) != 0 and who in err() and "2^24" in err()


def test_frontend_table_and_gather_argument_checks():
    L = N.lib

    def sinus(freq=FAKE, table=FAKE, T=1030, half=160):
        return L.esmk_op_sinus_table(freq, table, T, half, 2, None)

    def rope(freq=FAKE, cos=FAKE, sin=FAKE, T=1030, half=32):
        return L.esmk_op_rope_table(freq, cos, sin, T, half, None)

    for fn, who, nulls in ((sinus, "esmk_op_sinus_table", (dict(freq=None), dict(table=None))),
                           (rope, "esmk_op_rope_table", (dict(freq=None), dict(cos=None), dict(sin=None)))):
        for kw in nulls:
            assert fn(**kw) != 0 and who + ": null argument" in err(), (who, kw)
        for kw in (dict(T=0), dict(half=0), dict(T=-5)):
            assert fn(**kw) != 0 and who + ": T and half must be positive" in err(), (who, kw)
        assert fn(T=1 << 24, half=128) != 0 and who in err() and "2^31" in err()

    def gather(x=FAKE, sel=FAKE, out=FAKE, Nr=37, E=320, n=300):
        return L.esmk_op_gather_rows(x, sel, out, Nr, E, n, None)

    who = "esmk_op_gather_rows"
    for kw in (dict(x=None), dict(sel=None), dict(out=None)):
        assert gather(**kw) != 0 and who + ": null argument" in err(), kw
    for kw in (dict(Nr=0), dict(n=0), dict(n=-2), dict(Nr=(1 << 24) + 1)):
        assert gather(**kw) != 0 and who + ": N and n" in err(), kw
    for E in (0, 2, 322):
        assert gather(E=E) != 0 and who + ": E must be a positive multiple of 4" in err(), E


def test_linear_refuses_the_bits_of_the_closed_timing_experiments():
    """esmk_op_linear: bits 12..19 of operand_dtype once selected kernels with parts removed; any of them set is refused
    with a message of its own, before the call looks at a pointer or reaches a launch (the buffers are fake)."""
    f16 = N.dtype_code(torch.float16)
    for bit in range(12, 20):
        for extra in (0, 0x200, 1 << 28):  # alone, with the force_old hook, with forced half-height tiles
            rc = N.lib.esmk_op_linear(FAKE, FAKE, None, FAKE, 300, 320, 192, N.EPI_STORE_T, f16 | (1 << bit) | extra, None)
            assert rc != 0 and "esmk_op_linear: bits 12..19" in err(), (bit, extra, err())
    rc = N.lib.esmk_op_linear(FAKE, FAKE, None, FAKE, 300, 320, 192, N.EPI_STORE_T, f16 | 0xff000, None)
    assert rc != 0 and "esmk_op_linear: bits 12..19" in err()
    # without those bits the same call gets past that check: a bad epilogue is what it is refused for
    rc = N.lib.esmk_op_linear(FAKE, FAKE, None, FAKE, 300, 320, 192, 5, f16, None)
    assert rc != 0 and "bad epilogue" in err()


def test_layernorm_variant_selector_checks():
    """esmk_op_layernorm / esmk_op_layernorm_ex: the kernel has two forms, variant 0 (plain) and 7 (the engine's, also the
    default); every other selector (operand_dtype bits 8..11 = variant + 1) is refused before any launch.  Selectors
    default, 0 and 7 get past that check: with rows = 0 the calls are refused for the rows, not for the variant (still no
    launch; the buffers are fake)."""
    f16, bf16 = N.dtype_code(torch.float16), N.dtype_code(torch.bfloat16)

    def plain(variant, rows=9, E=320, dt=f16):
        code = dt | (0 if variant is None else (variant + 1) << 8)
        return N.lib.esmk_op_layernorm(FAKE, FAKE, FAKE, FAKE, None, rows, E, code, None)

    def ex(variant, rows=9, E=320, dt=f16):
        code = dt | (0 if variant is None else (variant + 1) << 8)
        return N.lib.esmk_op_layernorm_ex(FAKE, FAKE, FAKE, FAKE, None, rows, E, code, None, 0, 0, 0, 0, 1e-5, None)

    for call, who in ((plain, "esmk_op_layernorm: variant"), (ex, "esmk_op_layernorm_ex: variant")):
        for variant in (1, 2, 3, 4, 5, 6, 8, 14):
            for dt in (f16, bf16):
                assert call(variant, dt=dt) != 0 and who in err(), (variant, err())
        for variant in (None, 0, 7):
            assert call(variant, rows=0) != 0 and "variant" not in err(), (variant, err())
