"""Attention maps of token-packed batches without a GPU: argument checks and workspace sizes of
esmk_packed_workspace_bytes_maps / esmk_forward_packed_maps and of the two packed attention op entries (every check
below fails before the library touches the HIP runtime, see test_c_abi_validation_cpu.py), and the refusals the older
packed entries keep."""
import ctypes

import torch

from esm_amd import _native as N

FAKE = ctypes.c_void_p(0x1000)
BIG = 1 << 40


def make(L=2, E=128, H=2, **kw):
    cfg = N.EsmkConfig(L, E, H, 4 * E, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0, N.lib.esmk_last_error()
    return h


def err():
    return N.lib.esmk_last_error().decode()


def segs(lengths):
    out, row = [], 0
    for n in lengths:
        out += [row, n]
        row += (n + 15) // 16 * 16
    rows = max(64, (row + 127) // 128 * 128)
    return (ctypes.c_int32 * len(out))(*out), len(lengths), rows


LAYERS = (ctypes.c_int32 * 1)(2)
OUTS = (ctypes.c_void_p * 1)(0x2000)


def forward_maps(h, seg, rows=128, flags=N.OUT_ATTN, attn=FAKE, elems=BIG, contacts=FAKE, ws=16):
    arr = (ctypes.c_int32 * len(seg))(*seg)
    return N.lib.esmk_forward_packed_maps(h, FAKE, FAKE, arr, len(seg) // 2, rows, LAYERS, 1, OUTS, flags, FAKE, attn,
                                          ctypes.c_size_t(elems), contacts, FAKE, ctypes.c_size_t(ws), None)


def test_map_buffer_checks():
    h = make()  # L H = 4
    need = 4 * (20 * 20 + 5 * 5)
    for flags in (N.OUT_ATTN, N.OUT_ATTN_LOWP, N.OUT_ATTN | N.OUT_ATTN_LOWP, N.OUT_ATTN | N.OUT_CONTACTS | N.OUT_LOGITS):
        assert forward_maps(h, [0, 20, 32, 5], flags=flags, attn=None) != 0 and "attention buffer missing" in err()
        assert forward_maps(h, [0, 20, 32, 5], flags=flags, elems=need - 1) != 0 and "attention buffer too small" in err()
        assert forward_maps(h, [0, 20, 32, 5], flags=flags, elems=0) != 0 and "attention buffer too small" in err()
        # a buffer of exactly L H sum(len^2) elements passes this check: the next refusal is the workspace
        assert forward_maps(h, [0, 20, 32, 5], flags=flags, elems=need) != 0 and "workspace too small" in err()
    # without a map flag the buffer is not looked at: the _ex behaviour
    assert forward_maps(h, [0, 20, 32, 5], flags=N.OUT_CONTACTS, attn=None, elems=0) != 0 and "workspace too small" in err()
    assert forward_maps(h, [0, 20, 32, 5], flags=N.OUT_CONTACTS, attn=None, elems=0, contacts=None, ws=BIG) != 0
    assert "contacts buffer missing" in err()
    N.lib.esmk_destroy(h)


def test_segment_table_and_workspace_refusals():
    h = make()
    assert forward_maps(h, [0, 20, 32, 5], rows=100) != 0 and "multiple of 64" in err()
    assert forward_maps(h, [0, 0]) != 0 and "empty segment" in err()
    assert forward_maps(h, [0, 20, 24, 5]) != 0 and "multiples of 16" in err()
    assert forward_maps(h, [16, 20]) != 0 and "start at row 0" in err()
    assert forward_maps(h, [0, 40, 32, 5]) != 0 and "disjoint" in err()
    assert forward_maps(h, [0, 20, 112, 30]) != 0 and "past the last row" in err()
    assert forward_maps(h, [0, 20, 32, 5], flags=N.OUT_ATTN | N.OUT_COL_ATTN) != 0 and "ESMK_OUT_ATTN" in err()
    n = ctypes.c_size_t()
    arr = (ctypes.c_int32 * 4)(0, 20, 32, 5)
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, 2, 128, N.OUT_ATTN | N.OUT_COL_ATTN, ctypes.byref(n)) != 0
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, 2, 100, N.OUT_ATTN, ctypes.byref(n)) != 0 and "multiple of 64" in err()
    assert N.lib.esmk_packed_workspace_bytes_maps(h, None, 2, 128, N.OUT_ATTN, ctypes.byref(n)) != 0 and "null" in err()
    for flags in (N.OUT_ATTN, N.OUT_ATTN_LOWP, N.OUT_ATTN | N.OUT_CONTACTS | N.OUT_LOGITS):
        assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, 2, 128, flags, ctypes.byref(n)) == 0, err()
        assert forward_maps(h, [0, 20, 32, 5], flags=flags, ws=n.value - 1) != 0 and "workspace too small" in err()
    N.lib.esmk_destroy(h)


def test_families_without_a_packed_form_are_refused():
    arr = (ctypes.c_int32 * 2)(0, 20)
    n = ctypes.c_size_t()
    h = make(weight_split=4)
    assert forward_maps(h, [0, 20, 32, 5], ws=BIG) != 0 and "f16x3" in err()
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, 1, 64, N.OUT_ATTN, ctypes.byref(n)) != 0 and "f16x3" in err()
    N.lib.esmk_destroy(h)
    h = make(no_rope=2, token_dropout=0)
    assert forward_maps(h, [0, 20, 32, 5], ws=BIG) != 0 and "ESM-1" in err()
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, 1, 64, N.OUT_ATTN, ctypes.byref(n)) != 0 and "ESM-1" in err()
    N.lib.esmk_destroy(h)
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    assert N.lib.esmk_packed_workspace_bytes_maps(hm, arr, 1, 64, N.OUT_ATTN, ctypes.byref(n)) != 0 and "ESM-2 handle" in err()
    assert forward_maps(hm, [0, 20], rows=64, ws=BIG) != 0 and "ESM-2 handle" in err()
    N.lib.esmk_destroy(hm)


def test_workspace_does_not_grow_with_tmax_squared():
    """650M dims, one 1022-token sequence with 63 of 100 tokens: the map flag adds the row log-sum-exp [H, rows] (which
    the contact flag brings as well) and the map offsets — nothing of the size of a map."""
    h = make(L=33, E=1280, H=20)
    mix = [1022] + [100] * 63
    arr, n, rows = segs(mix)
    maps, ex, plain, both = (ctypes.c_size_t() for _ in range(4))
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, n, rows, N.OUT_ATTN, ctypes.byref(maps)) == 0, err()
    assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, n, rows, N.OUT_CONTACTS, ctypes.byref(ex)) == 0, err()
    assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, n, rows, 0, ctypes.byref(plain)) == 0, err()
    assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, n, rows, N.OUT_ATTN | N.OUT_CONTACTS, ctypes.byref(both)) == 0
    lse = 20 * rows * 4
    print(f"\nworkspace: maps {maps.value}, contacts (_ex) {ex.value}, neither {plain.value}, lse {lse}")
    assert maps.value <= ex.value + lse
    assert plain.value < maps.value <= plain.value + lse + 8 * n + 1024  # lse + uint64 offsets (+ alignment)
    assert both.value <= ex.value + 8 * n + 1024
    one_map = 1022 * 1022 * 4
    assert maps.value - plain.value < one_map
    # without a map flag: the _ex sizes exactly
    for flags in (0, N.OUT_LOGITS, N.OUT_CONTACTS, N.OUT_CONTACTS | N.OUT_LOGITS | N.OUT_REPR_LOWP):
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert N.lib.esmk_packed_workspace_bytes_maps(h, arr, n, rows, flags, ctypes.byref(a)) == 0
        assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, n, rows, flags, ctypes.byref(b)) == 0
        assert a.value == b.value
    N.lib.esmk_destroy(h)


def test_older_entries_keep_refusing_maps():
    h = make()
    arr = (ctypes.c_int32 * 4)(0, 20, 32, 5)
    n = ctypes.c_size_t()
    for flags in (N.OUT_ATTN, N.OUT_ATTN_LOWP, N.OUT_ATTN | N.OUT_CONTACTS):
        assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, 2, 128, flags, ctypes.byref(n)) != 0
        assert "attention maps take padded batches" in err()
        assert N.lib.esmk_forward_packed_ex(h, FAKE, FAKE, arr, 2, 128, LAYERS, 1, OUTS, flags, FAKE, FAKE, FAKE,
                                            ctypes.c_size_t(BIG), None) != 0
        assert "attention maps take padded batches" in err()
        assert N.lib.esmk_packed_workspace_bytes(h, 2, 128, flags, ctypes.byref(n)) != 0 and "ESMK_OUT_LOGITS" in err()
        assert N.lib.esmk_forward_packed(h, FAKE, FAKE, arr, 2, 128, LAYERS, 1, OUTS, flags, FAKE, FAKE,
                                         ctypes.c_size_t(BIG), None) != 0 and "padded batches" in err()
    N.lib.esmk_destroy(h)


def _op_attention(seg, rows=128, Tp=192, H=2, D=64, dt=1, q=FAKE, bias_k=None, bias_v=None, ctx=FAKE):
    arr = (ctypes.c_int32 * len(seg))(*seg) if seg is not None else None
    return N.lib.esmk_op_attention_packed(q, FAKE, FAKE, None, arr, len(seg) // 2 if seg else 1, rows, Tp, H, D, dt,
                                          bias_k, bias_v, ctx, None, None)


def _op_probs(seg, rows=128, H=2, D=64, L=3, layer=0, dt=1, lowp=0, out=FAKE, elems=BIG, lse=FAKE):
    arr = (ctypes.c_int32 * len(seg))(*seg) if seg is not None else None
    return N.lib.esmk_op_attention_probs_packed(FAKE, FAKE, lse, None, arr, len(seg) // 2 if seg else 1, rows, H, D, L,
                                                layer, dt, lowp, out, ctypes.c_size_t(elems), None)


def test_packed_op_entries_validate_before_the_runtime():
    ok = [16, 20, 48, 5]  # a gap in front of the first segment is allowed here
    assert _op_attention(ok, q=None) != 0 and "null argument" in err()
    assert _op_attention(ok, ctx=None) != 0 and "null argument" in err()
    assert _op_attention(ok, bias_k=FAKE) != 0 and "bias_k / bias_v must be null" in err()
    assert _op_attention(ok, bias_v=FAKE) != 0 and "bias_k / bias_v must be null" in err()
    assert _op_attention(ok, D=32) != 0 and "head_dim" in err()
    assert _op_attention(ok, dt=0) != 0 and "operand_dtype" in err()
    assert _op_attention(ok, H=0) != 0
    assert _op_attention(None) != 0 and "segment table" in err()
    assert _op_attention(ok, rows=100) != 0 and "multiple of 64" in err()
    assert _op_attention([0, 20, 24, 5]) != 0 and "multiples of 16" in err()
    assert _op_attention([0, 40, 32, 5]) != 0 and "disjoint" in err()
    assert _op_attention([0, 20, 112, 30]) != 0 and "past the last row" in err()
    assert _op_attention([0, 0]) != 0 and "empty segment" in err()
    assert _op_attention(ok, Tp=128) != 0 and "rows + 64" in err()
    assert _op_attention(ok, Tp=200) != 0 and "rows + 64" in err()

    need = 3 * 2 * (20 * 20 + 5 * 5)
    assert _op_probs(ok, lse=None) != 0 and "null argument" in err()
    assert _op_probs(ok, out=None) != 0 and "attention buffer missing" in err()
    assert _op_probs(ok, elems=need - 1) != 0 and "attention buffer too small" in err()
    assert _op_probs(ok, layer=3) != 0 and "layer out of range" in err()
    assert _op_probs(ok, layer=-1) != 0 and "layer out of range" in err()
    assert _op_probs(ok, D=96) != 0 and "head_dim" in err()
    assert _op_probs(ok, dt=0) != 0 and "operand_dtype" in err()
    assert _op_probs([0, 20, 24, 5]) != 0 and "multiples of 16" in err()
    assert _op_probs([0, 20, 16, 5]) != 0 and "disjoint" in err()
    assert _op_probs(ok, rows=1 << 25) != 0 and "2^24" in err()
