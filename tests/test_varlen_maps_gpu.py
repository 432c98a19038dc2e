"""Attention maps of token-packed batches (esmk_forward_packed_maps / ESM2.forward_varlen(need_head_weights=True)) on
the MI355X.

The packed map kernel computes every element exactly as the padded one does (same MFMAs in the same order, the same
log-sum-exp), so the contract is bit-equality: the unpacked tensor IS ``forward(need_head_weights=True)["attentions"]``,
and every ragged per-sequence view is that sequence run alone.  Against the reference the maps keep the bound
tests/test_model_gpu.py holds the padded maps to."""
import argparse
import glob
import os

import pytest
import torch

import esm
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict

pytestmark = pytest.mark.gpu
PAD, MASK, CLS, EOS = 1, 32, 0, 2
# the committed ESM-2 fixtures of the reference that carry "attentions" (tests/test_model_gpu.py loads the same files)
GOLDEN = [p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "esm2_*.pt")))
          if torch.load(p, weights_only=False)["attentions"] is not None]

# on and next to the 32-row wave, 64-key tile and 128-row workgroup edges
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]
MASKS = [(11, 5), (11, 40), (8, 7), (3, 30)]
INTERIOR_PAD = [(11, 100), (11, 101), (9, 64), (10, 3), (5, 30)]


def build(L, E, H, seed):
    m = esm.ESM2(L, E, H).eval()
    m.load_state_dict(synth_esm2_state_dict(L, E, H, seed=seed))
    return m.cuda()


def build_esm1b(L, E, H, ln_before):
    args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                              max_positions=1024, token_dropout=True, emb_layer_norm_before=ln_before)
    model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    model.load_state_dict(synth_esm1b_state_dict(L, E, H, seed=1, ln_before=ln_before), strict=True)
    return model.cuda()


def ragged_batch(lengths, seed, masks=(), interior_pad=()):
    """Right-padded [B, max len] batch as BatchConverter yields it: <cls> residues <eos> <pad>..."""
    g = torch.Generator().manual_seed(seed)
    toks = torch.full((len(lengths), max(lengths)), PAD, dtype=torch.int64)
    for b, n in enumerate(lengths):
        toks[b, 0] = CLS
        if n > 2:
            toks[b, 1:n - 1] = torch.randint(4, 24, (n - 2,), generator=g)
        toks[b, n - 1] = EOS
    for b, t in masks:
        toks[b, t] = MASK
    for b, t in interior_pad:
        toks[b, t] = PAD
    return toks


def check_packed_maps(model, toks, lengths, L, alone=True):
    """The whole contract on one batch: unpacked tensor == padded forward's, ragged views == each sequence alone, exact
    zeros on <pad> rows / columns, and representations / logits untouched by the map request."""
    dev = toks.cuda()
    with torch.no_grad():
        model.forward_varlen(toks, repr_layers=[L], min_saving=None, need_head_weights=True)
        # every byte of the workspace = 0xFF (NaN): nothing may be read before it is written
        model._engine.workspace.fill_(255)
        pk = model.forward_varlen(toks, repr_layers=[0, L], min_saving=None, need_head_weights=True)
        pd = model(dev, repr_layers=[0, L], need_head_weights=True)
        plain = model.forward_varlen(toks, repr_layers=[0, L], min_saving=None)
        raw = model.forward_varlen(toks, repr_layers=[0, L], min_saving=None, unpack=False, need_head_weights=True)
    assert pk["attentions"].shape == pd["attentions"].shape and pk["attentions"].dtype == pd["attentions"].dtype
    assert torch.isfinite(pk["attentions"]).all()
    assert torch.equal(pk["attentions"], pd["attentions"])
    for layer in (0, L):
        assert torch.equal(pk["representations"][layer], plain["representations"][layer])
    assert torch.equal(pk["logits"], plain["logits"])
    pad = dev.eq(PAD)
    assert (pk["attentions"].permute(0, 3, 1, 2, 4)[pad] == 0).all()   # <pad> query rows
    assert (pk["attentions"].permute(0, 4, 1, 2, 3)[pad] == 0).all()   # <pad> key columns
    views = raw["attentions"]
    H = pd["attentions"].shape[2]
    assert len(views) == len(lengths)
    for b, n in enumerate(lengths):
        assert views[b].shape == (L, H, n, n)
        assert torch.equal(views[b], pd["attentions"][b, :, :, :n, :n]), (b, n)
        if alone:
            with torch.no_grad():
                one = model(dev[b:b + 1, :n], need_head_weights=True)["attentions"][0]
            assert torch.equal(views[b], one), (b, n)
    # the views share one flat buffer, back to back
    assert all(views[b + 1].data_ptr() == views[b].data_ptr() + views[b].numel() * views[b].element_size()
               for b in range(len(lengths) - 1))


@pytest.mark.parametrize("dims,fold", [((2, 128, 2), "1"), ((2, 128, 2), "0"), ((2, 256, 2), "0"), ((2, 320, 20), "1")],
                         ids=["d64_fold", "d64_nofold", "d128", "d16_fold"])
def test_packed_maps_bit_equal(monkeypatch, dims, fold):
    monkeypatch.setenv("ESM_AMD_LN_FOLD", fold)
    L, E, H = dims
    model = build(L, E, H, seed=11)
    toks = ragged_batch(LENGTHS, seed=3, masks=MASKS, interior_pad=INTERIOR_PAD)
    check_packed_maps(model, toks, LENGTHS, L)
    assert model.ln_fold_active() == (fold == "1")
    assert model.supports_varlen_maps


@pytest.mark.parametrize("ln_before", [True, False], ids=["esm1b", "esm1v_style"])
def test_packed_maps_esm1b(ln_before):
    L, E, H = 2, 128, 2
    model = build_esm1b(L, E, H, ln_before)
    lengths = [40, 2, 150, 65, 300, 128, 1]
    toks = ragged_batch(lengths, seed=8, masks=[(0, 3), (4, 77)], interior_pad=[(2, 30), (4, 64)])
    check_packed_maps(model, toks, lengths, L)


@pytest.mark.parametrize("fold", ["1", "0"], ids=["fold", "nofold"])
@pytest.mark.parametrize("dt,dims", [(torch.float16, (2, 128, 2)), (torch.bfloat16, (2, 128, 2)), (torch.float16, (2, 256, 2))],
                         ids=["fp16_d64", "bf16_d64", "fp16_d128"])
def test_packed_maps_low_precision_models(monkeypatch, dt, dims, fold):
    """``.half()`` / ``.bfloat16()`` models: the maps come back in the model dtype, written natively by the kernel
    (ESMK_OUT_ATTN_LOWP) — the same bits as fp32 maps + a cast (ESM_AMD_NATIVE_LOWP=0)."""
    L, E, H = dims
    if E // H == 128 and fold == "1":
        fold = "0"  # the fold exists for head_dim <= 64
    monkeypatch.setenv("ESM_AMD_LN_FOLD", fold)
    model = build(L, E, H, seed=7).to(dt)
    lengths = [33, 2, 129, 64, 200, 1]
    toks = ragged_batch(lengths, seed=5, masks=[(2, 9)], interior_pad=[(4, 50)])
    monkeypatch.setenv("ESM_AMD_NATIVE_LOWP", "1")
    check_packed_maps(model, toks, lengths, L, alone=False)
    with torch.no_grad():
        native = model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True)["attentions"]
        monkeypatch.setenv("ESM_AMD_NATIVE_LOWP", "0")
        cast = model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True)["attentions"]
    for a, b in zip(native, cast):
        assert a.dtype == b.dtype == dt and torch.equal(a, b)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_packed_maps_against_reference_fixture(path):
    """The reference's own attentions (tests/golden/make_golden.py): the bound of test_engine_matches_reference_fixture,
    5e-3 absolute, and exact zeros wherever the reference has them."""
    fix = torch.load(path, weights_only=False)
    d = fix["dims"]
    model = build(d["L"], d["E"], d["H"], d["seed"])
    with torch.no_grad():
        out = model.forward_varlen(fix["tokens"], min_saving=None, need_head_weights=True)
    a = out["attentions"].cpu()
    err = (a - fix["attentions"]).abs().max().item()
    print(f"\n{os.path.basename(path)}: packed attention err {err:.2e}")
    assert err < 5e-3
    assert (a[fix["attentions"] == 0] == 0).all()


def test_some_fixture_carries_attentions():
    assert len(GOLDEN) >= 2


def test_map_offsets_past_2_31_elements():
    """53 sequences of 1022 tokens and a short one, 2 layers x 20 heads: 2.2e9 map elements (4.4 GB of fp16) in front of the
    last sequence.  The element offsets are 64-bit prefix sums: the one place where the packed map buffer passes 2^31
    elements.  (tests/test_index_width_ops_gpu.py and tests/test_index_width_engine_gpu.py take the tensors of the padded
    kernels, of packed attention and of the layer loop past 2^31 and 2^32 bytes; the packed map and contact kernels are held
    by this test alone.)"""
    L, E, H = 2, 1280, 20
    model = build(L, E, H, seed=3).half()
    lengths = [1022] * 53 + [77]
    assert L * H * sum(n * n for n in lengths[:-1]) > 2 ** 31
    toks = ragged_batch(lengths, seed=2, masks=[(52, 500), (53, 9)])
    with torch.no_grad():
        views = model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True)["attentions"]
        assert views[0].dtype == torch.float16
        assert (views[-1].data_ptr() - views[0].data_ptr()) // 2 > 2 ** 31
        for b in (52, 53, 0):
            n = lengths[b]
            one = model(toks[b:b + 1, :n].cuda(), need_head_weights=True)["attentions"][0]
            assert torch.equal(views[b], one), b
            rows = views[b].float().sum(-1)
            assert (rows - 1).abs().max().item() < 2e-2  # fp16 maps of up to 1022 keys
    del views
    torch.cuda.empty_cache()


def test_contacts_and_maps_together():
    L, E, H = 2, 128, 2
    model = build(L, E, H, seed=11)
    toks = ragged_batch(LENGTHS, seed=3, masks=MASKS, interior_pad=INTERIOR_PAD)
    with torch.no_grad():
        ct = model.forward_varlen(toks, repr_layers=[L], min_saving=None, contacts_only=True)
        maps = model.forward_varlen(toks, repr_layers=[L], min_saving=None, need_head_weights=True)
        both = model.forward_varlen(toks, repr_layers=[L], min_saving=None, need_head_weights=True, return_contacts=True)
        only = model.forward_varlen(toks, repr_layers=[L], min_saving=None, need_head_weights=True, contacts_only=True)
        raw = model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True, return_contacts=True)
        raw_ct = model.forward_varlen(toks, min_saving=None, unpack=False, contacts_only=True)
    assert torch.equal(both["contacts"], ct["contacts"]) and torch.equal(only["contacts"], ct["contacts"])
    assert torch.equal(both["attentions"], maps["attentions"]) and torch.equal(only["attentions"], maps["attentions"])
    assert torch.equal(both["logits"], maps["logits"]) and "logits" not in only
    assert torch.equal(both["representations"][L], ct["representations"][L])
    for a, b in zip(raw["contacts"], raw_ct["contacts"]):
        assert torch.equal(a, b)
    # a .half() model: native fp16 maps next to the (fp32-accumulated) fused contacts
    half = build(L, E, H, seed=11).half()
    with torch.no_grad():
        ct = half.forward_varlen(toks, min_saving=None, contacts_only=True)
        both = half.forward_varlen(toks, min_saving=None, need_head_weights=True, return_contacts=True)
        maps = half.forward_varlen(toks, min_saving=None, need_head_weights=True)
    assert both["attentions"].dtype == torch.float16
    assert torch.equal(both["contacts"], ct["contacts"]) and torch.equal(both["attentions"], maps["attentions"])


def test_fallback_to_padded_forward_keeps_the_maps():
    model = build(1, 128, 2, seed=2)
    toks = ragged_batch([40, 40, 39], seed=1)
    with torch.no_grad():
        a = model.forward_varlen(toks, repr_layers=[1], need_head_weights=True)                   # nothing to save: padded
        b = model.forward_varlen(toks, repr_layers=[1], min_saving=None, need_head_weights=True)  # forced packing
        c = model.forward_varlen(toks, repr_layers=[1], need_head_weights=True, return_contacts=True)
        d = model.forward_varlen(toks, repr_layers=[1])
    assert torch.equal(a["attentions"], b["attentions"]) and torch.equal(c["attentions"], b["attentions"])
    assert "attentions" not in d
    with torch.no_grad():
        ct = model(toks.cuda(), contacts_only=True)["contacts"]
    assert torch.equal(c["contacts"], ct)


def test_c_abi_flags_on_the_device():
    """ESMK_OUT_ATTN_LOWP alone implies the maps; without a map flag the entry is esmk_forward_packed_ex."""
    import ctypes

    from esm_amd import _native as N
    from esm_amd.packing import pack_plan

    L, E, H = 2, 128, 2
    model = build(L, E, H, seed=11)
    lengths = [33, 2, 129]
    toks = ragged_batch(lengths, seed=5)
    with torch.no_grad():
        ref = model.forward_varlen(toks, min_saving=None, unpack=False, need_head_weights=True)["attentions"]
    eng = model._engine
    plan = pack_plan(toks, PAD)
    idx, _ = plan.index("cuda")
    flat = plan.pack(toks, PAD, idx)
    seg_ptr = ctypes.cast(plan.segments.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    n = L * H * sum(x * x for x in lengths)
    op_dt = eng.operand_dtype
    out = torch.zeros(n, dtype=op_dt, device="cuda")
    logits = torch.empty((plan.rows, 33), device="cuda")
    need = ctypes.c_size_t()
    flags = N.OUT_LOGITS | N.OUT_ATTN_LOWP
    N.check(N.lib.esmk_packed_workspace_bytes_maps(eng.handle, seg_ptr, 3, plan.rows, flags, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    N.check(N.lib.esmk_forward_packed_maps(eng.handle, N.ptr(eng.packed), N.ptr(flat), seg_ptr, 3, plan.rows, None, 0, None,
                                           flags, N.ptr(logits), N.ptr(out), n, None, N.ptr(ws), ws.numel(),
                                           N.cur_stream()))
    torch.cuda.synchronize()
    got = torch.cat([v.reshape(-1) for v in ref])
    assert torch.equal(out, got.to(op_dt))
