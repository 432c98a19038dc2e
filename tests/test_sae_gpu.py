"""``model.sae_features`` (esm_amd/sae.py) through synthetic models of esm_amd/synth.py — ESM-2 with L = 3, E = 128, H = 2, one
ESM-2 with E = 96 (Ep = 128 != E: zero pad columns in both operand images) and one ESM-1b — with random SAEs of F = 256 (every row
selects in LDS) and F = 4160 (about half the features active: every row goes through the radix select), in both LayerNorm-fold
settings.

The call is held bit for bit against the chain of single ops (tests/test_sae_ops_gpu.py holds each of those against numpy)
applied to the rows of ``forward(repr_layers=[layer])``; everything else — batch independence, chunking, varlen, selectors,
stream edits — is equality of bits as well.  The one inexact statement (how far a steered feature rises) uses the product bound
of tests/test_precision_ops_gpu.py::test_f16x3_product."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _contract as C
import _sae_ref as ref
import _stream_edit_ref as R
import esm
import esm_amd
from esm_amd import SparseAutoencoder, StreamEdit
from esm_amd import _native as nat
from esm_amd import ops
from esm_amd.interventions import plan_edits
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
L, B, T = 3, 3, 41
DIMS = {"esm2": (128, 2), "esm2_96": (96, 6), "esm1b": (128, 2)}
FOLD = pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def state(kind):
    E, H = DIMS[kind]
    return synth_esm1b_state_dict(L, E, H, seed=5) if kind == "esm1b" else synth_esm2_state_dict(L, E, H, seed=11)


@functools.lru_cache(maxsize=None)
def model_of(kind):
    E, H = DIMS[kind]
    if kind == "esm1b":
        args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                                  max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
        model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
    else:
        model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(state(kind), strict=True)
    return model.cuda()


def in_mode(kind, fold, monkeypatch):
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1" if fold else "0")
    model = model_of(kind)
    model(batch().cuda())
    assert model.ln_fold_active() is fold
    return model


def batch(pads=True, seed=12, b=B, t=T):
    toks = synth_tokens(b, t - 2, seed=seed)
    if pads:
        toks[1, 30] = 2
        toks[1, 31:] = 1
    return toks


@functools.lru_cache(maxsize=None)
def sae_of(E, F, activation="relu", k=None, scale=0.37):
    """a random SAE with tied, row-normalised decoder: about half of the features of a row are active"""
    g = torch.Generator().manual_seed(F + E)
    w_enc = torch.randn(F, E, generator=g) / E ** 0.5
    b_enc = 0.05 * torch.randn(F, generator=g)
    w_dec = w_enc / w_enc.norm(dim=1, keepdim=True)
    b_dec = 0.1 * torch.randn(E, generator=g)
    thr = torch.where(torch.rand(F, generator=g) < 0.5, 0.0, 0.02)
    return SparseAutoencoder(w_enc, b_enc, w_dec, b_dec, activation=activation, k=k, threshold=thr, input_scale=scale)


def rows_of(toks, positions, model):
    t = toks.cpu().numpy()
    keep = t != model.padding_idx
    if positions == "residues":
        keep &= (t != model.cls_idx) & (t != model.eos_idx)
    return np.argwhere(keep).astype(np.int32)


def chain(model, toks, sae, rep, top_k, positions="residues", k_sae=0):
    """the op chain on the rows of a captured representation, with operand images built here"""
    Bt, Tt = toks.shape
    rows = rows_of(toks, positions, model)
    flat = torch.from_numpy(rows[:, 0] * Tt + rows[:, 1]).to(torch.int32).cuda()
    w, b, thr = sae.padded()
    w3 = torch.zeros((sae.Fp, 3 * sae.Ep), dtype=torch.float16, device="cuda")
    ops.split_weight_ex(w.cuda(), w3, sae.Ep, 3)
    x = rep.reshape(Bt * Tt, sae.E).float().contiguous()
    a3 = ops.sae_rows(x, flat, None if sae.b_dec is None else sae.b_dec.cuda(), sae.input_scale)
    z = ops.linear(a3, w3, b.cuda(), nat.EPI_STORE_F32)
    out = ops.sae_topk(z, top_k, thr.cuda(), k_sae=k_sae)
    return dict(rows=torch.from_numpy(rows).cuda(), indices=out["indices"], values=out["values"], n_active=out["n_active"],
                dense=z[:, :sae.F].contiguous(), a3=a3, w3=w3)


def same(a, b, keys=("rows", "indices", "values", "n_active"), what=""):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key)
        assert torch.equal(a[key], b[key]), (what, key)


def of_sequence(out, b):
    """the rows of sequence b"""
    m = out["rows"][:, 0] == b
    return {k: (out[k][m] if k != "rows" else out[k][m][:, 1]) for k in ("rows", "indices", "values", "n_active")}


# ---- 1. the call is the chain of ops ----------------------------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", list(DIMS))
def test_against_the_op_chain(kind, fold, monkeypatch):
    model, toks = in_mode(kind, fold, monkeypatch), batch().cuda()
    E = DIMS[kind][0]
    radix = 0
    for F in (256, 4160):
        sae = sae_of(E, F)
        for layer in (0, 1, L):
            rep = model(toks, repr_layers=[layer])["representations"][layer]
            want = chain(model, toks, sae, rep, 32)
            got = model.sae_features(toks, sae, layer, return_dense=True, protein_max=True)
            same(got, want, what=(F, layer))
            assert torch.equal(got["dense"], want["dense"]), (F, layer)
            # the returned top-k is esmk_op_sae_topk of the returned dense
            again = ops.sae_topk(got["dense"].contiguous(), 32, sae.threshold.cuda())
            assert torch.equal(again["indices"], got["indices"]) and torch.equal(again["values"], got["values"])
            assert torch.equal(again["n_active"], got["n_active"])
            # and what the numpy restatement selects from it; the per-protein maxima are its segment maxima
            dense = got["dense"].cpu().numpy()
            ri, rv, rc = ref.topk(dense, sae.threshold.numpy(), 32)
            assert np.array_equal(got["indices"].cpu().numpy(), ri) and np.array_equal(got["values"].cpu().numpy(), rv)
            assert np.array_equal(got["n_active"].cpu().numpy(), rc)
            pm, pa = ref.segment_max(dense, sae.threshold.numpy(), got["rows"].cpu().numpy(), B)
            assert np.array_equal(got["protein_max"].cpu().numpy(), pm) and np.array_equal(got["protein_argmax"].cpu().numpy(), pa)
            assert got["protein_max"].shape == (B, F) and (pa >= 0).any() and got["rows"].shape[0] == want["rows"].shape[0] > 0
            radix += int((rc > ops.sae_cand()).sum())
            assert 0 < rc.min() and rc.max() < F  # a mix of active and inactive features in every row
    assert radix > 0  # F = 4160: rows with more actives than the LDS candidates hold went through the radix select
    assert esm_amd.sae_features(model, toks, sae_of(E, 256), 1)["indices"].shape[1] == 32


# ---- 2. a sequence's features do not depend on its batch ---------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_batch_independence(kind, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    sae = sae_of(DIMS[kind][0], 256)
    toks = batch(pads=False, seed=40, b=5)
    lens = [41, 17, 30, 41, 9]
    for b, n in enumerate(lens):
        toks[b, n - 1] = 2
        toks[b, n:] = 1
    toks = toks.cuda()
    full = model.sae_features(toks, sae, L, protein_max=True)
    for b, n in enumerate(lens):
        alone = model.sae_features(toks[b:b + 1, :n].contiguous(), sae, L, protein_max=True)
        assert alone["rows"].shape[0] == n - 2
        same(of_sequence(alone, 0), of_sequence(full, b), what=b)
        assert torch.equal(alone["protein_max"][0], full["protein_max"][b]) and torch.equal(alone["protein_argmax"][0], full["protein_argmax"][b])


# ---- 3. chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["relu", "topk"])
def test_chunks_give_the_same_bits(activation, monkeypatch):
    from esm_amd.sae import plan_chunks

    model = in_mode("esm2", True, monkeypatch)
    sae = sae_of(128, 4160) if activation == "relu" else sae_of(128, 4160, "topk", 24)
    toks = batch(pads=False, seed=41, b=8, t=102)
    toks[3, 60] = 2
    toks[3, 61:] = 1
    toks = toks.cuda()
    one = model.sae_features(toks, sae, 1, top_k=16, protein_max=True)
    n = one["rows"].shape[0]
    small = 256 * (6 * sae.Ep + 4 * sae.Fp) + 100
    assert len(plan_chunks(n, sae.F, sae.E, small)) >= 3 and len(plan_chunks(n, sae.F, sae.E, 2 << 30)) == 1
    many = model.sae_features(toks, sae, 1, top_k=16, protein_max=True, max_bytes=small)
    same(many, one, keys=("rows", "indices", "values", "n_active", "protein_max", "protein_argmax"))
    with pytest.raises(ValueError, match="max_bytes"):
        model.sae_features(toks, sae, 1, max_bytes=1000)
    with pytest.raises(ValueError, match="return_dense"):
        model.sae_features(toks, sae, 1, return_dense=True, max_bytes=small)


# ---- 4. token-packed forward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_varlen_is_the_padded_call(kind, monkeypatch):
    model = in_mode(kind, True, monkeypatch)
    sae = sae_of(DIMS[kind][0], 256)
    toks = batch(pads=False, seed=42, b=4)
    for b, n in enumerate([41, 12, 25, 33]):
        toks[b, n - 1] = 2
        toks[b, n:] = 1
    toks = toks.cuda()
    padded = model.sae_features(toks, sae, 2, protein_max=True)
    packed = model.sae_features(toks, sae, 2, protein_max=True, varlen=True)
    same(packed, padded, keys=("rows", "indices", "values", "n_active", "protein_max", "protein_argmax"))


# ---- 5. selectors -------------------------------------------------------------------------------------------------------------
def test_positions_all_against_residues(monkeypatch):
    model, toks = in_mode("esm2", True, monkeypatch), batch().cuda()
    sae = sae_of(128, 256)
    res = model.sae_features(toks, sae, L, positions="residues")
    every = model.sae_features(toks, sae, L, positions="all")
    t = toks.cpu()
    assert every["rows"].shape[0] == int(t.ne(1).sum()) and res["rows"].shape[0] == int((t.ne(1) & t.ne(0) & t.ne(2)).sum())
    rows_all = every["rows"].cpu()
    tok_of = t[rows_all[:, 0].long(), rows_all[:, 1].long()]
    assert bool((tok_of != 1).all()) and bool((tok_of == 0).any()) and bool((tok_of == 2).any())
    inner = ((tok_of != 0) & (tok_of != 2)).cuda()
    for key in ("rows", "indices", "values", "n_active"):
        assert torch.equal(every[key][inner], res[key]), key
    # ascending (sequence, position)
    flat = rows_all[:, 0].long() * T + rows_all[:, 1].long()
    assert bool((flat[1:] > flat[:-1]).all())


# ---- 6. a top-k autoencoder ---------------------------------------------------------------------------------------------------
def test_topk_autoencoder(monkeypatch):
    model, toks = in_mode("esm2", True, monkeypatch), batch().cuda()
    relu, top = sae_of(128, 256), sae_of(128, 256, "topk", 12)
    dense = model.sae_features(toks, relu, 1, return_dense=True)["dense"].cpu().numpy()
    # a threshold that leaves some rows with fewer than k actives
    hard = SparseAutoencoder(top.w_enc, top.b_enc, top.w_dec, top.b_dec, activation="topk", k=12,
                             threshold=float(np.sort(dense, axis=1)[:, -8].mean().clip(min=0.0)), input_scale=top.input_scale)
    for sae in (top, hard):
        out = model.sae_features(toks, sae, 1, protein_max=True)
        assert out["indices"].shape[1] == 12  # top_k None: the SAE's k
        count = ref.active_mask(dense, sae.threshold.numpy()).sum(1)
        filled = (out["indices"] >= 0).sum(1).cpu().numpy()
        assert np.array_equal(filled, np.minimum(12, count)) and np.array_equal(out["n_active"].cpu().numpy(), np.minimum(12, count))
        assert bool(((out["values"] == 0) == (out["indices"] < 0)).all())
        ri, rv, rc = ref.topk(dense, sae.threshold.numpy(), 12, k_sae=12)
        assert np.array_equal(out["indices"].cpu().numpy(), ri) and np.array_equal(out["values"].cpu().numpy(), rv)
        pm, pa = ref.segment_max(dense, sae.threshold.numpy(), out["rows"].cpu().numpy(), B, k_sae=12)
        assert np.array_equal(out["protein_max"].cpu().numpy(), pm) and np.array_equal(out["protein_argmax"].cpu().numpy(), pa)
        fewer = model.sae_features(toks, sae, 1, top_k=5)
        assert torch.equal(fewer["indices"], out["indices"][:, :5]) and torch.equal(fewer["n_active"], out["n_active"])
    assert (ref.active_mask(dense, hard.threshold.numpy()).sum(1) < 12).any()
    with pytest.raises(ValueError, match="exceeds"):
        model.sae_features(toks, top, 1, top_k=13)


# ---- 7. under stream edits ----------------------------------------------------------------------------------------------------
@FOLD
def test_stream_edits_are_seen(fold, monkeypatch):
    model, toks = in_mode("esm2", fold, monkeypatch), batch().cuda()
    sae = sae_of(128, 256)
    base = model.sae_features(toks, sae, 1, return_dense=True)
    f = int(base["indices"][0, 3])
    edit = StreamEdit(1, "add", value=sae.direction(f), gain=3.0)
    rep_e = model.forward_edited(toks, [edit], repr_layers=[1])["representations"][1]
    rep_b = model(toks, repr_layers=[1])["representations"][1]
    with model.stream_edits([edit]):
        inside = model.sae_features(toks, sae, 1, return_dense=True)
    want = chain(model, toks, sae, rep_e, 32)
    same(inside, want)
    assert torch.equal(inside["dense"], want["dense"])
    same(model.sae_features(toks, sae, 1), base)  # and the context is gone afterwards

    # the rise of feature f: the exact three-term sums of the restated images, fp64, within the two product bounds
    w3 = ref.weight_image(sae.padded()[0].numpy()).astype(np.float64)[f]
    b_enc = float(sae.b_enc[f])
    rows = base["rows"].cpu().numpy()

    def three(rep):
        x = rep.reshape(B * T, -1).float().cpu().numpy()[rows[:, 0] * T + rows[:, 1]]
        a3 = ref.image_rows(ref.u_rows(x, None, sae.b_dec.numpy(), sae.input_scale)).astype(np.float64)
        return a3 @ w3 + b_enc, (3 * sae.Ep + 2) * U * (np.abs(a3) @ np.abs(w3) + abs(b_enc)), x

    z_b, bound_b, x_b = three(rep_b)
    z_e, bound_e, x_e = three(rep_e)
    rise = inside["dense"][:, f].double().cpu().numpy() - base["dense"][:, f].double().cpu().numpy()
    ratio = (np.abs(rise - (z_e - z_b)) / (bound_b + bound_e)).max()
    full = (ref.z64(x_e, sae.w_enc.numpy(), sae.b_enc.numpy(), sae.b_dec.numpy(), sae.input_scale)[:, f]
            - ref.z64(x_b, sae.w_enc.numpy(), sae.b_enc.numpy(), sae.b_dec.numpy(), sae.input_scale)[:, f])
    # what steering by 3 direction(f) predicts: 3 <w_enc[f], w_dec[f]> (input_scale and inv_scale cancel)
    predicted = 3.0 * float(sae.w_enc[f].double() @ sae.w_dec[f].double())
    print(f"\nsae steering, feature {f}: rise {rise.min():.4f} .. {rise.max():.4f}, predicted {predicted:.4f}; {ratio:.3f} of the "
          f"product bounds; three-term against unsplit operands {np.abs((z_e - z_b) - full).max():.2e}")
    assert ratio <= 1.0, ratio
    assert predicted > 0.5 and np.abs(full - predicted).max() < 1e-4 * predicted  # x' = x + 3 d, rounded to fp32 once per element
    assert rise.min() > 0.99 * predicted


# ---- 8. splicing the reconstruction in ----------------------------------------------------------------------------------------
@FOLD
def test_splice_reconstruction(fold, monkeypatch):
    model = in_mode("esm2", fold, monkeypatch)
    E, H = DIMS["esm2"]
    sae = sae_of(E, 256)
    toks = batch(pads=False, seed=43)
    out = model.sae_features(toks.cuda(), sae, 1, top_k=64, positions="all")
    assert out["rows"].shape[0] == B * T
    xhat = sae.decode(out["indices"], out["values"])
    restated = ref.decode(out["indices"].cpu().numpy(), out["values"].cpu().numpy(), sae.w_dec.numpy(), sae.b_dec.numpy(), sae.input_scale)
    assert np.array_equal(xhat.cpu().numpy().view(np.uint32), restated.view(np.uint32))
    edits = [StreamEdit(1, "set", value=torch.from_numpy(restated).reshape(B, T, E))]
    got = model.forward_edited(toks.cuda(), [StreamEdit(1, "set", value=xhat.reshape(B, T, E))], repr_layers=[1])
    assert torch.equal(got["representations"][1].float().reshape(B * T, E), xhat)
    plans = plan_edits(model, edits, B, T)
    want = R.forward_edited_ref(state("esm2"), toks, L, H, edits=plans, repr_layers=[1])
    floor = C.floor_forward(state("esm2"), toks, L, H, model=model, forward=R.forward_edited_ref, edits=plans, repr_layers=[1])
    C.check_tensors(f"sae splice {'fold' if fold else 'plain'} logits", got["logits"], want["logits"], floor["logits"], toks.ne(1),
                    deep=False)
