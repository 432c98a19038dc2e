"""The host side of esm_amd/sae.py and of the esmk_op_sae_* entries (include/esmk.h): checkpoint spellings, the padding of F,
every refusal that needs no GPU, the chunk planner, the command line's parser, and tests/_sae_ref.py against a plain torch
computation in fp64."""
import ctypes

import numpy as np
import pytest
import torch

import _sae_ref as ref
import esm
import esm_amd
from esm_amd import SparseAutoencoder, _native as N
from esm_amd import sae as S

FAKE = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1004)


def err():
    return N.lib.esmk_last_error().decode()


def parts(F=100, E=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(w_enc=torch.randn(F, E, generator=g), b_enc=torch.randn(F, generator=g), w_dec=torch.randn(F, E, generator=g),
                b_dec=torch.randn(E, generator=g))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_both_checkpoint_spellings(tmp_path):
    p = parts()
    a = {"encoder.weight": p["w_enc"], "encoder.bias": p["b_enc"], "decoder.weight": p["w_dec"].t().contiguous(), "bias": p["b_dec"]}
    b = {"W_enc": p["w_enc"].t().contiguous(), "b_enc": p["b_enc"], "W_dec": p["w_dec"], "b_dec": p["b_dec"]}
    torch.save(a, tmp_path / "a.pt")
    for sd in (a, b, str(tmp_path / "a.pt")):
        sae = SparseAutoencoder.from_state_dict(sd, input_scale=0.5)
        assert (sae.F, sae.E, sae.activation, sae.k, sae.input_scale) == (100, 64, "relu", None, 0.5)
        for key in ("w_enc", "b_enc", "w_dec", "b_dec"):
            assert torch.equal(getattr(sae, key), p[key]), key
        assert torch.equal(sae.threshold, torch.zeros(100))
    top = SparseAutoencoder.from_state_dict(b, activation="topk", k=16, threshold=0.25)
    assert (top.activation, top.k) == ("topk", 16) and bool((top.threshold == 0.25).all())
    with pytest.raises(ValueError, match=r"found \['enc', 'something'\]"):
        SparseAutoencoder.from_state_dict({"enc": p["w_enc"], "something": p["b_enc"]})


def test_padding_of_F():
    p = parts(F=100)
    thr = torch.rand(100)
    sae = SparseAutoencoder(**p, threshold=thr)
    assert (sae.F, sae.Fp, sae.Ep) == (100, 128, 64)
    w, b, t = sae.padded()
    assert w.shape == (128, 64) and torch.equal(w[:100], p["w_enc"]) and bool((w[100:] == 0).all())
    assert torch.equal(b[:100], p["b_enc"]) and bool((b[100:] == 0).all())
    assert torch.equal(t[:100], thr) and bool(torch.isinf(t[100:]).all()) and bool((t[100:] > 0).all())
    # z of a padding feature is 0 + 0: never above +inf, and the restatement never reports it
    z = np.zeros((1, 128), dtype=np.float32)
    assert not ref.active_mask(z, t.numpy())[0, 100:].any()
    wide = SparseAutoencoder(torch.zeros(64, 96), torch.zeros(64))  # E = 96: columns padded to 128 with zeros
    assert wide.Ep == 128 and wide.padded()[0].shape == (64, 128)
    assert SparseAutoencoder(torch.zeros(128, 64), torch.zeros(128)).Fp == 128


def test_inv_scale_and_direction():
    p = parts()
    sae = SparseAutoencoder(**p, input_scale=0.37)
    assert sae.inv_scale == float(np.float32(1.0 / 0.37))
    d = sae.direction(7)
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), np.float32(1.0 / 0.37) * p["w_dec"][7].numpy())
    with pytest.raises(ValueError):
        sae.direction(100)
    with pytest.raises(ValueError, match="no decoder"):
        SparseAutoencoder(p["w_enc"], p["b_enc"]).direction(0)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    p = parts()
    with pytest.raises(ValueError, match=">= 0"):
        SparseAutoencoder(**p, threshold=-0.1)
    with pytest.raises(ValueError, match=">= 0"):
        SparseAutoencoder(**p, threshold=torch.full((100,), float("nan")))
    t = torch.zeros(100)
    t[3] = -1e-9
    with pytest.raises(ValueError, match=">= 0"):
        SparseAutoencoder(**p, threshold=t)
    with pytest.raises(ValueError, match="65536"):
        SparseAutoencoder(torch.zeros(65537, 4), torch.zeros(65537))
    SparseAutoencoder(torch.zeros(65536, 4), torch.zeros(65536))
    with pytest.raises(ValueError, match="k in 1 .. 256"):
        SparseAutoencoder(**p, activation="topk")
    with pytest.raises(ValueError, match="k in 1 .. 256"):
        SparseAutoencoder(**p, activation="topk", k=257)
    with pytest.raises(ValueError, match="goes with"):
        SparseAutoencoder(**p, k=8)
    with pytest.raises(ValueError, match="activation"):
        SparseAutoencoder(**p, activation="jumprelu")
    with pytest.raises(ValueError, match="input_scale"):
        SparseAutoencoder(**p, input_scale=0.0)
    with pytest.raises(ValueError, match="b_enc has shape"):
        SparseAutoencoder(p["w_enc"], torch.zeros(99))
    with pytest.raises(ValueError, match="w_dec has shape"):
        SparseAutoencoder(p["w_enc"], p["b_enc"], p["w_dec"].t())


def test_call_refusals():
    model = esm.ESM2(2, 64, 2).eval()  # on the CPU: every refusal below comes before the engine is asked for
    toks = torch.zeros(1, 8, dtype=torch.int64)
    sae = SparseAutoencoder(**parts())
    top = SparseAutoencoder(**parts(), activation="topk", k=16)
    with pytest.raises(ValueError, match="embed_dim"):
        model.sae_features(toks, SparseAutoencoder(**parts(E=128)), 1)
    for layer in (-1, 3):
        with pytest.raises(ValueError, match="outside 0 .. 2"):
            model.sae_features(toks, sae, layer)
    for k in (0, 257):
        with pytest.raises(ValueError, match="1 .. 256"):
            model.sae_features(toks, sae, 1, top_k=k)
    with pytest.raises(ValueError, match="exceeds the 16"):
        model.sae_features(toks, top, 1, top_k=17)
    with pytest.raises(ValueError, match="positions"):
        model.sae_features(toks, sae, 1, positions="cls")
    with pytest.raises(TypeError):
        model.sae_features(toks, {"W_enc": None}, 1)
    with pytest.raises(NotImplementedError, match="window"):
        esm_amd.sae_features(model, toks, sae, 1, window=1024)
    with pytest.raises(RuntimeError, match="MI355X"):  # everything is in order: the CPU model itself is what is refused
        model.sae_features(toks, sae, 1)


def test_msa_transformer_refuses():
    import argparse

    args = argparse.Namespace(layers=1, embed_dim=64, ffn_embed_dim=256, attention_heads=2, max_positions=64, max_tokens_per_msa=2 ** 14,
                              embed_positions_msa=True, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer"))
    with pytest.raises(NotImplementedError, match="MSA Transformer"):
        esm_amd.sae_features(msa, torch.zeros(1, 2, 8, dtype=torch.int64), SparseAutoencoder(**parts()), 1)
    assert not hasattr(msa, "sae_features")


def test_exports():
    assert esm_amd.SparseAutoencoder is S.SparseAutoencoder
    assert callable(esm_amd.sae_features) and esm_amd.sae_features.sae_features is S.sae_features
    assert esm.ProteinBertModel.sae_features is esm.ESM2.sae_features


# ---- the chunk planner -------------------------------------------------------------------------------------------------------
def test_chunk_planner():
    F, E = 10240, 1280
    per_row = 6 * 1280 + 4 * 10240
    assert S.plan_chunks(65408, F, E, 2 << 30) == [(0, 44032), (44032, 21376)]
    assert (2 << 30) // per_row // 256 * 256 == 44032 and 44032 * per_row <= 2 << 30 < (44032 + 256) * per_row
    assert S.plan_chunks(1000, F, E, 2 << 30) == [(0, 1000)]
    assert S.plan_chunks(0, F, E, 2 << 30) == []
    chunks = S.plan_chunks(1000, F, E, 256 * per_row)
    assert chunks == [(0, 256), (256, 256), (512, 256), (768, 232)]
    with pytest.raises(ValueError, match="max_bytes"):
        S.plan_chunks(1000, F, E, 256 * per_row - 1)
    # a returned dense matrix comes out of the same budget
    assert S.plan_chunks(1000, F, E, 512 * per_row + 7, dense_bytes=256 * per_row) == chunks
    # F and E are padded to 64 in the scratch
    assert S.plan_chunks(300, 100, 96, 256 * (6 * 128 + 4 * 128)) == [(0, 256), (256, 44)]
    for lo, c in S.plan_chunks(10 ** 6, 65536, 1280, 2 << 30)[:-1]:
        assert c % 256 == 0 and c * (6 * 1280 + 4 * 65536) <= 2 << 30


# ---- the restatement against plain torch, fp64 ---------------------------------------------------------------------------------
def test_reference_against_torch_dense():
    F, E, n, k = 200, 64, 23, 16
    p = parts(F, E, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, E, generator=g)
    thr = torch.where(torch.rand(F, generator=g) < 0.5, 0.0, 0.3)
    scale = 0.37
    z = ref.z64(x.numpy(), p["w_enc"].numpy(), p["b_enc"].numpy(), p["b_dec"].numpy(), scale)
    u = (torch.tensor(scale) * x - p["b_dec"]).double()  # fp32 operations, one rounding each
    zt = u @ p["w_enc"].double().t() + p["b_enc"].double()
    assert np.abs(z - zt.numpy()).max() < 1e-12
    z32 = z.astype(np.float32)
    acts = torch.where(torch.from_numpy(z32) > thr, torch.from_numpy(z32), torch.zeros(()))
    tv, ti = torch.topk(acts, k, dim=1)
    idx, val, cnt = ref.topk(z32, thr.numpy(), k)
    assert np.array_equal(cnt, (acts > 0).sum(1).numpy()) and cnt.min() >= k  # (no ties, at least k actives: torch.topk's order is defined)
    assert np.array_equal(val, tv.numpy()) and np.array_equal(idx, ti.numpy().astype(np.int32))
    # ties go to the lower index, unused slots are -1 / 0, NaN is never active, +inf is
    zz = np.array([[1.0, 2.0, 2.0, np.nan, -np.inf, np.inf, 0.5, 0.0]], dtype=np.float32)
    idx, val, cnt = ref.topk(zz, np.array([0, 0, 0, 0, 0, 0, 0.5, 0], dtype=np.float32), 6)
    assert idx.tolist() == [[5, 1, 2, 0, -1, -1]] and val[0, 3:].tolist() == [1.0, 0.0, 0.0] and cnt.tolist() == [4]
    assert ref.topk(zz, 0.0, 2, k_sae=3)[2].tolist() == [3] and ref.kept_mask(zz, 0.0, 3)[0].tolist() == [0, 1, 1, 0, 0, 1, 0, 0]
    # per-sequence maxima: the lowest position wins a tie
    rows = np.array([[0, 1], [0, 2], [1, 1]], dtype=np.int32)
    zs = np.array([[1.0, -1.0, 0.2], [1.0, -2.0, 0.4], [0.5, -1.0, 0.0]], dtype=np.float32)
    pm, pa = ref.segment_max(zs, 0.0, rows, 2)
    assert pm.tolist() == [[1.0, 0.0, 0.4000000059604645], [0.5, 0.0, 0.0]] and pa.tolist() == [[1, -1, 2], [1, -1, -1]]
    dense = torch.where(torch.from_numpy(zs) > 0, torch.from_numpy(zs), torch.zeros(()))
    assert torch.equal(torch.from_numpy(pm[0]), dense[:2].amax(0))
    # decode against torch in fp64, and its fill rule
    di = np.array([[2, 0, -1], [-1, -1, -1]], dtype=np.int32)
    dv = np.array([[1.5, 0.25, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    out = ref.decode(di, dv, p["w_dec"].numpy(), p["b_dec"].numpy(), scale)
    want = (p["b_dec"].double() + 1.5 * p["w_dec"][2].double() + 0.25 * p["w_dec"][0].double()) / scale
    assert np.abs(out[0] - want.numpy()).max() < 1e-5 and np.array_equal(out[1], np.float32(1.0 / scale) * p["b_dec"].numpy())
    # the operand image: hi | hi | lo per 64 columns, pads zero, hi + lo within 2^-21 of u
    img = ref.image_rows(np.linspace(-3, 3, 2 * 96, dtype=np.float32).reshape(2, 96)).reshape(2, 2, 3, 64)
    assert np.array_equal(img[:, :, 0], img[:, :, 1]) and (img[:, 1, :, 32:] == 0).all()
    back = (img[:, :, 0].astype(np.float64) + img[:, :, 2].astype(np.float64)).reshape(2, 128)[:, :96]
    assert np.abs(back - np.linspace(-3, 3, 2 * 96, dtype=np.float32).reshape(2, 96)).max() < 3 * 2.0 ** -21


# ---- the C entries: refused before any HIP call, on fake pointers ------------------------------------------------------------
def test_op_entries_refuse_before_any_hip_call():
    L = N.lib
    assert L.esmk_op_sae_cand() >= 256  # the LDS path holds at least the largest k

    def rows(x=FAKE, ldx=128, n_x=9, lst=FAKE, n=4, b=FAKE, scale=1.0, img=FAKE, ld=384, E=128):
        return L.esmk_op_sae_rows(x, ldx, n_x, lst, n, b, scale, img, ld, E, None)

    for kw, msg in ((dict(x=None), "null"), (dict(img=None), "null"), (dict(E=126, ldx=128), "multiple of 4"), (dict(E=0), "multiple of 4"),
                    (dict(ldx=124), "ldx"), (dict(ldx=130), "ldx"), (dict(ld=380), "ld_image"), (dict(ld=386), "ld_image"),
                    (dict(E=96, ld=3 * 96), "ld_image"), (dict(n_x=0), "N"), (dict(n=-1), "n"), (dict(lst=None, n=10), "exceed"),
                    (dict(scale=float("inf")), "finite"), (dict(scale=float("nan")), "finite"), (dict(x=ODD), "aligned"),
                    (dict(b=ODD), "aligned")):
        assert rows(**kw) != 0 and msg in err(), (kw, err())
    assert rows(n=0) == 0

    def topk(z=FAKE, ldz=256, thr=FAKE, t=0.0, n=3, F=256, k=8, k_sae=0, idx=FAKE, val=FAKE, cnt=FAKE, cut=None, path=None):
        return L.esmk_op_sae_topk(z, ldz, thr, t, n, F, k, k_sae, idx, val, cnt, cut, path, None)

    for kw, msg in ((dict(z=None), "null"), (dict(idx=None), "null"), (dict(val=None), "null"), (dict(cnt=None), "null"),
                    (dict(F=65540, ldz=65540), "65536"), (dict(F=0), "65536"), (dict(F=254), "65536"), (dict(k=0), "1 .. 256"),
                    (dict(k=257), "1 .. 256"), (dict(k_sae=257), "k_sae"), (dict(k=9, k_sae=8), "k_sae"), (dict(k_sae=-1), "k_sae"),
                    (dict(ldz=252), "ldz"), (dict(ldz=258), "ldz"), (dict(n=-1), "n"), (dict(thr=None, t=-0.5), "negative"),
                    (dict(thr=None, t=float("nan")), "negative"), (dict(z=ODD), "aligned"), (dict(thr=ODD), "aligned"),
                    (dict(cut=ODD), "aligned")):
        assert topk(**kw) != 0 and msg in err(), (kw, err())
    assert topk(n=0) == 0 and topk(n=0, F=65536, ldz=65536, k=256, k_sae=256) == 0

    def seg(z=FAKE, ldz=256, thr=FAKE, t=0.0, cut=None, rw=FAKE, st=FAKE, row0=0, n=3, F=256, B=2, pm=FAKE, pa=FAKE):
        return L.esmk_op_sae_segment_max(z, ldz, thr, t, cut, rw, st, row0, n, F, B, pm, pa, None)

    for kw, msg in ((dict(z=None), "null"), (dict(rw=None), "null"), (dict(st=None), "null"), (dict(pm=None), "null"),
                    (dict(pa=None), "null"), (dict(F=65537, ldz=65537), "65536"), (dict(F=0), "65536"), (dict(B=0), "B"),
                    (dict(n=-1), "n"), (dict(row0=-1), "row0"), (dict(ldz=255), "ldz"), (dict(thr=None, t=-1.0), "negative"),
                    (dict(cut=ODD), "aligned")):
        assert seg(**kw) != 0 and msg in err(), (kw, err())
    assert seg(n=0) == 0

    def dec(idx=FAKE, val=FAKE, n=3, k=8, w=FAKE, b=FAKE, inv=1.0, out=FAKE, E=128, F=256):
        return L.esmk_op_sae_decode(idx, val, n, k, w, b, inv, out, E, F, None)

    for kw, msg in ((dict(idx=None), "null"), (dict(val=None), "null"), (dict(w=None), "null"), (dict(out=None), "null"),
                    (dict(E=126), "multiple of 4"), (dict(E=0), "multiple of 4"), (dict(F=65537), "65536"), (dict(F=0), "65536"),
                    (dict(k=0), "1 .. 256"), (dict(k=257), "1 .. 256"), (dict(n=-1), "n"), (dict(w=ODD), "aligned"), (dict(out=ODD), "aligned")):
        assert dec(**kw) != 0 and msg in err(), (kw, err())
    assert dec(n=0) == 0


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_cli_parser():
    from esm_amd import sae_features as cli

    base = ["--model-location", "m.pt", "--sae", "sae.pt", "--layer", "24", "--output-dir", "out"]
    a = cli.parse_args(base + ["--sequence", "MKV"])
    assert (a.model_location, a.sae, a.layer, a.sequence, a.fasta, a.output_dir) == ("m.pt", "sae.pt", 24, "MKV", None, "out")
    assert (a.top_k, a.positions, a.protein_max, a.varlen) == (None, "residues", False, True)
    b = cli.parse_args(base + ["--fasta", "x.fasta", "--top-k", "64", "--positions", "all", "--protein-max", "--no-varlen"])
    assert (b.fasta, b.top_k, b.positions, b.protein_max, b.varlen) == ("x.fasta", 64, "all", True, False)
    for bad in (base, base + ["--sequence", "MKV", "--fasta", "x.fasta"], base[2:] + ["--sequence", "MKV"],
                base + ["--sequence", "MKV", "--positions", "cls"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert cli.main is S.main
