"""Contacts of token-packed batches without a GPU: argument checks and workspace sizes of esmk_packed_workspace_bytes_ex /
esmk_forward_packed_ex (every check below fails before the library touches the HIP runtime, see
test_c_abi_validation_cpu.py), and the extraction driver's dispatch."""
import ctypes

import torch

from esm_amd import _native as N

FAKE = ctypes.c_void_p(0x1000)


def make(L=2, E=128, H=2, **kw):
    cfg = N.EsmkConfig(L, E, H, 4 * E, 33, 1, 32, 0, 2, 1, 1, 1, N.dtype_code(torch.float16), 0, 0, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    assert N.lib.esmk_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
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


def ws_bytes(h, lengths, flags):
    arr, n, rows = segs(lengths)
    b = ctypes.c_size_t()
    assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, n, rows, flags, ctypes.byref(b)) == 0, err()
    return b.value


def test_refusals():
    h = make()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)

    def call(seg, rows=128, flags=N.OUT_CONTACTS, contacts=FAKE, ws=16):
        arr = (ctypes.c_int32 * len(seg))(*seg)
        return N.lib.esmk_forward_packed_ex(h, FAKE, FAKE, arr, len(seg) // 2, rows, layers, 1, outs, flags, FAKE,
                                            contacts, FAKE, ctypes.c_size_t(ws), None)

    assert call([0, 20, 32, 5], flags=N.OUT_CONTACTS | N.OUT_ATTN) != 0 and "attention maps" in err()
    assert call([0, 20, 32, 5], flags=N.OUT_ATTN_LOWP) != 0 and "attention maps" in err()
    assert call([0, 20, 32, 5], contacts=None) != 0 and "contacts buffer missing" in err()
    assert call([0, 20, 32, 5], rows=100) != 0 and "multiple of 64" in err()
    assert call([0, 0]) != 0 and "empty segment" in err()
    assert call([0, 20, 24, 5]) != 0 and "multiples of 16" in err()
    assert call([16, 20]) != 0 and "start at row 0" in err()
    assert call([0, 40, 32, 5]) != 0 and "disjoint" in err()
    assert call([0, 20, 112, 30]) != 0 and "past the last row" in err()
    assert call([0, 20, 32, 5]) != 0 and "workspace too small" in err()
    n = ctypes.c_size_t()
    arr = (ctypes.c_int32 * 4)(0, 20, 32, 5)
    assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, 2, 128, N.OUT_CONTACTS | N.OUT_ATTN, ctypes.byref(n)) != 0
    assert N.lib.esmk_packed_workspace_bytes_ex(h, arr, 2, 128, N.OUT_CONTACTS, ctypes.byref(n)) == 0
    assert call([0, 20, 32, 5], ws=n.value - 1) != 0 and "workspace too small" in err()
    # the padded-only entry keeps its message
    assert N.lib.esmk_forward_packed(h, FAKE, FAKE, arr, 2, 128, layers, 1, outs, N.OUT_CONTACTS, FAKE, FAKE,
                                     ctypes.c_size_t(1 << 40), None) != 0 and "padded batches" in err()
    N.lib.esmk_destroy(h)
    h = make(weight_split=4)
    assert call([0, 20, 32, 5], ws=1 << 40) != 0 and "f16x3" in err()
    N.lib.esmk_destroy(h)


def test_msa_handle_refused():
    cfg = N.EsmkMsaConfig(2, 128, 2, 256, 33, 1, 32, 0, 2, 1, 0, 1026, 1, N.dtype_code(torch.float16))
    hm = ctypes.c_void_p()
    assert N.lib.esmk_msa_create(ctypes.byref(cfg), ctypes.byref(hm)) == 0
    arr = (ctypes.c_int32 * 2)(0, 20)
    n = ctypes.c_size_t()
    assert N.lib.esmk_packed_workspace_bytes_ex(hm, arr, 1, 64, N.OUT_CONTACTS, ctypes.byref(n)) != 0
    assert "ESM-2 handle" in err()
    layers = (ctypes.c_int32 * 1)(2)
    outs = (ctypes.c_void_p * 1)(0x2000)
    assert N.lib.esmk_forward_packed_ex(hm, FAKE, FAKE, arr, 1, 64, layers, 1, outs, N.OUT_CONTACTS, FAKE, FAKE, FAKE,
                                        ctypes.c_size_t(1 << 40), None) != 0 and "ESM-2 handle" in err()
    N.lib.esmk_destroy(hm)


def test_workspace_size():
    h = make(L=33, E=1280, H=20)
    # without contacts: the entry without the segment table
    for flags in (N.OUT_LOGITS, N.OUT_LOGITS | N.OUT_REPR_LOWP, 0):
        arr, n, rows = segs([100, 300, 17])
        b = ctypes.c_size_t()
        assert N.lib.esmk_packed_workspace_bytes(h, n, rows, flags, ctypes.byref(b)) == 0
        assert ws_bytes(h, [100, 300, 17], flags) == b.value
    # grows with sum(len^2) at a fixed row count
    a = ws_bytes(h, [128] * 8, N.OUT_CONTACTS)
    b = ws_bytes(h, [512, 512], N.OUT_CONTACTS)
    assert b > a
    assert ws_bytes(h, [2, 2, 2], N.OUT_CONTACTS) < ws_bytes(h, [6, 2, 2], N.OUT_CONTACTS)
    # one long sequence batched with many short ones: at most half of the padded batch's workspace
    mix = [1022] + [100] * 63
    padded = ctypes.c_size_t()
    assert N.lib.esmk_workspace_bytes(h, len(mix), max(mix), N.OUT_CONTACTS, ctypes.byref(padded)) == 0
    packed = ws_bytes(h, mix, N.OUT_CONTACTS)
    print(f"\nworkspace: packed {packed / 2**20:.0f} MiB, padded {padded.value / 2**20:.0f} MiB")
    assert packed <= padded.value // 2
    N.lib.esmk_destroy(h)


def test_extract_dispatch_packed_contacts():
    from esm_amd.extract import make_embed_fn

    calls = []

    class Engine:
        supports_varlen = True
        supports_contacts_only = True
        supports_varlen_contacts = True

        def forward_varlen(self, toks, repr_layers, lengths=None, contacts_only=False):
            calls.append(("varlen", tuple(repr_layers), lengths, contacts_only))
            return {}

        def __call__(self, toks, repr_layers, return_contacts=False, contacts_only=False):
            calls.append(("forward", tuple(repr_layers), return_contacts, contacts_only))
            return {}

    toks = torch.zeros((2, 5), dtype=torch.int64)
    make_embed_fn(Engine())(toks, [3], True, lengths=[5, 4])
    make_embed_fn(Engine())(toks, [3], False, lengths=[5, 4])
    make_embed_fn(Engine(), varlen=False)(toks, [3], True)
    assert calls == [("varlen", (3,), [5, 4], True), ("varlen", (3,), [5, 4], False), ("forward", (3,), False, True)]
