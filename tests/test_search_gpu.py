"""Protein search (esm_amd/search.py) through the synthetic models of esm_amd/synth.py — ESM-2 with L = 3 and E = 128 or E = 96,
in both LayerNorm-fold settings, and one ESM-1b: the early exit ``model.embed_layer`` against ``forward``'s representation bit
for bit, its launch counts, the handle's limit and its refusals; ``model.pool`` against the numpy reference and across the ways
to batch; the index (build, file, search against the numpy top-k and fp64, blocks, exclude_self), ``search_and_align`` against
the aligner run by hand, and the command line."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _align_ref as aref
import _search_ref as ref
import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import search as S
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict, synth_msa_state_dict, synth_msa_tokens, synth_tokens

pytestmark = pytest.mark.gpu
L = 3
DIMS = {"esm2": (128, 2), "esm2_96": (96, 6), "esm1b": (128, 2)}
FOLD = pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
KINDS = pytest.mark.parametrize("kind", list(DIMS))
LENS = [39, 17, 30, 1]
GEMMS = ("gemm_qkv_rope", "gemm_out_proj", "gemm_fc1_gelu", "gemm_fc2")


@functools.lru_cache(maxsize=None)
def model_of(kind):
    E, H = DIMS[kind]
    if kind == "esm1b":
        args = argparse.Namespace(arch="roberta_large", layers=L, embed_dim=E, ffn_embed_dim=4 * E, attention_heads=H,
                                  max_positions=1024, token_dropout=True, emb_layer_norm_before=True)
        model = esm.ProteinBertModel(args, esm.Alphabet.from_architecture("roberta_large")).eval()
        model.load_state_dict(synth_esm1b_state_dict(L, E, H, seed=5), strict=True)
    else:
        model = esm.ESM2(L, E, H).eval()
        model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=11), strict=True)
    return model.cuda()


def tokens_of(lengths, seed):
    toks = synth_tokens(len(lengths), max(lengths), seed=seed)
    for k, n in enumerate(lengths):
        toks[k, n + 1] = 2
        toks[k, n + 2:] = 1
    return toks


def in_mode(kind, fold, monkeypatch):
    monkeypatch.setenv("ESM_AMD_LN_FOLD", "1" if fold else "0")
    model = model_of(kind)
    model(tokens_of(LENS, 3).cuda())
    assert model.ln_fold_active() is fold
    return model


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


# ---- embed_layer ----------------------------------------------------------------------------------------------------------
@FOLD
@KINDS
def test_embed_layer_is_forwards_representation(kind, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    logits = model(toks)["logits"]
    for layer in (0, 1, L - 1, L, None):
        k = L if layer is None else layer
        want = model(toks, repr_layers=[k])["representations"][k]
        got = model.embed_layer(toks, layer)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(LENS), max(LENS) + 2, DIMS[kind][0])
        same_bits(got, want, (kind, fold, layer, "padded"))
        want = model.forward_varlen(toks, repr_layers=[k], min_saving=None)["representations"][k]
        same_bits(model.embed_layer(toks, layer, varlen=True), want, (kind, fold, layer, "varlen"))
        same_bits(model.embed_layer(toks.cpu(), layer, varlen=True), want, (kind, fold, layer, "varlen from the host"))
        # the limit is gone: the next forward is the usual one
        same_bits(model(toks)["logits"], logits, (kind, fold, layer, "logits afterwards"))


@FOLD
def test_embed_layer_runs_only_the_layers_below(fold, monkeypatch):
    model = in_mode("esm2", fold, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()

    def launches(call):
        model.profile_begin()
        call()
        return {e["name"]: e["launches"] for e in model.profile_end()}

    full = launches(lambda: model(toks, repr_layers=[1]))
    one = launches(lambda: model.embed_layer(toks, 1))
    two = launches(lambda: model.embed_layer(toks, 2))
    whole = launches(lambda: model.embed_layer(toks, L))
    for name in GEMMS:
        assert one.get(name, 0) > 0 and L * one[name] == full[name] == whole[name] and two[name] == 2 * one[name], (name, one, two, full)
    assert one.get("attention", 0) * L == full["attention"]
    for name in ("lm_head_dense", "lm_head_logits"):
        assert full.get(name, 0) > 0 and one.get(name, 0) == 0 and two.get(name, 0) == 0, (name, one, two, full)


def test_the_limit_is_cleared_after_an_exception(monkeypatch):
    model = in_mode("esm2", True, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    logits = model(toks)["logits"]
    eng = model._engine
    seen = []

    def boom(*args, **kwargs):
        seen.append(1)
        raise RuntimeError("boom")

    monkeypatch.setattr(eng, "forward", boom)
    with pytest.raises(RuntimeError, match="boom"):
        model.embed_layer(toks, 1)
    monkeypatch.undo()
    assert seen and model._engine is eng
    same_bits(model(toks)["logits"], logits, "logits after the exception")  # (refused by name if the limit were still set)


def test_limit_refusals(monkeypatch):
    model = in_mode("esm2", True, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    B, T = toks.shape
    E, H = DIMS["esm2"]
    logits = model(toks)["logits"]
    eng = model._engine
    dev = toks.device
    f32 = dict(dtype=torch.float32, device=dev)
    for bad in (-1, L + 1):
        with pytest.raises(N.EsmkError, match=r"esmk_set_layer_limit: n_layers must be 0 \(the whole stack\) .. 3"):
            eng.set_layer_limit(bad)
    eng.set_layer_limit(L)  # the whole stack
    same_bits(model(toks)["logits"], logits, "limit L")
    try:
        eng.set_layer_limit(1)
        lim = r"a layer limit of 1 is set \(esmk_set_layer_limit\)"
        with pytest.raises(N.EsmkError, match="esmk_forward: " + lim + ".*ESMK_OUT_LOGITS"):
            model(toks)
        with pytest.raises(N.EsmkError, match="esmk_forward: " + lim + ".*ESMK_OUT_CONTACTS"):
            model(toks, contacts_only=True)
        attn = torch.empty((B, L, H, T, T), **f32)
        for flag in (N.OUT_ATTN, N.OUT_ATTN_LOWP):
            with pytest.raises(N.EsmkError, match=lim + ".*ESMK_OUT_ATTN"):
                eng.forward(toks, [], [], flag, None, attn, None)
        rep = torch.empty((B, T, E), **f32)
        with pytest.raises(N.EsmkError, match=lim + ".*representation 2 is above it"):
            eng.forward(toks, [2], [rep], 0, None, None, None)
        eng.forward(toks, [1], [rep], 0, None, None, None)  # what the limit serves
        same_bits(rep, model.embed_layer(toks, 1), "representation 1 under a held limit")
        eng.set_layer_limit(1)
        whole = lim + ".*needs the whole stack"
        with pytest.raises(N.EsmkError, match="esmk_forward_rows: " + whole):
            model.masked_marginals(toks)
        with pytest.raises(N.EsmkError, match="esmk_forward_packed_rows: " + whole):
            model.masked_marginals(toks, varlen=True)
        with pytest.raises(N.EsmkError, match="esmk_forward_rows_contacts: " + whole):
            eng.forward_rows_contacts(toks, None, model.alphabet_size, T - 2)
        with pytest.raises(N.EsmkError, match="esmk_forward_packed_maps: " + whole):
            model.forward_varlen(toks, need_head_weights=True, min_saving=None)
        head = esm_amd.PairHead(torch.ones(2, L * H), torch.zeros(2), None, None)
        with pytest.raises(N.EsmkError, match="esmk_forward_rows_pair: " + whole):
            model.pair_logits(toks, head)
        with pytest.raises(N.EsmkError, match=lim + ".*ESMK_OUT_LOGITS"):
            model.forward_varlen(toks, min_saving=None)
        # a held edit above the limit
        edit = esm_amd.StreamEdit(2, "scale", None, gain=0.5, positions="residues")
        with model.stream_edits([edit]):
            model._engine_ready(dev)
            with pytest.raises(N.EsmkError, match=lim + ".*a stream edit at layer 2 is above it"):
                eng.forward(toks, [1], [rep], 0, None, None, None)
    finally:
        eng.set_layer_limit(0)
    same_bits(model(toks)["logits"], logits, "logits after the refusals")


def test_embed_layer_under_stream_edits(monkeypatch):
    model = in_mode("esm2", True, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    plain = model.embed_layer(toks, 2)
    early = esm_amd.StreamEdit(1, "scale", None, gain=0.5, positions="residues")
    at = esm_amd.StreamEdit(2, "scale", None, gain=0.5, positions="residues")
    late = esm_amd.StreamEdit(3, "scale", None, gain=0.5, positions="residues")
    for edits in ([early], [at], [early, at]):
        with model.stream_edits(edits):
            want = model(toks, repr_layers=[2])["representations"][2]
            got = model.embed_layer(toks, 2)
        same_bits(got, want, "edited")
        assert not torch.equal(got, plain)
    with model.stream_edits([early, late]):
        with pytest.raises(ValueError, match="the edit at layer 3 lies above"):
            model.embed_layer(toks, 2)
        with pytest.raises(ValueError, match="varlen=True inside model.stream_edits"):
            model.embed_layer(toks, 3, varlen=True)
        same_bits(model.embed_layer(toks, 3), model(toks, repr_layers=[3])["representations"][3], "every edit applies at L")
    same_bits(model.embed_layer(toks, 2), plain, "no edits afterwards")


def test_model_refusals(monkeypatch):
    model = in_mode("esm2", True, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    for call in (model.embed_layer, model.pool):
        with pytest.raises(NotImplementedError, match="window"):
            call(toks, 1, window=16)
        with pytest.raises(ValueError, match="outside 0 .. 3"):
            call(toks, 4)
    args = argparse.Namespace(layers=2, embed_dim=128, ffn_embed_dim=256, attention_heads=2, dropout=0.1, attention_dropout=0.1,
                              activation_dropout=0.1, max_positions=1024, embed_positions_msa=True, embed_positions_msa_dim=128,
                              max_tokens=2 ** 14, max_tokens_per_msa=2 ** 14)
    msa = esm.MSATransformer(args, esm.Alphabet.from_architecture("msa_transformer")).eval()
    for call in (msa.embed_layer, msa.pool, msa.search):
        with pytest.raises(NotImplementedError, match="MSA Transformer"):
            call(toks)
    msa.load_state_dict(synth_msa_state_dict(2, 128, 2, 256, seed=1), strict=True)
    msa = msa.cuda()
    msa(synth_msa_tokens(1, 4, 12, seed=2).cuda())
    assert N.lib.esmk_set_layer_limit(msa._engine.handle, 1) != 0
    assert "esmk_set_layer_limit: MSA handle" in N.lib.esmk_last_error().decode()


# ---- pool -----------------------------------------------------------------------------------------------------------------
@FOLD
@KINDS
def test_pool(kind, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    toks = tokens_of(LENS, 3).cuda()
    B, T = toks.shape
    E = DIMS[kind][0]
    rows = np.concatenate([b * T + 1 + np.arange(n) for b, n in enumerate(LENS)])
    off = np.concatenate([[0], np.cumsum(LENS)])
    for layer in (1, L):
        rep = model.embed_layer(toks, layer)
        want = torch.from_numpy(ref.pool_rows(rep.reshape(B * T, E).cpu().numpy(), rows, off)).cuda()
        got = model.pool(toks, layer)
        same_bits(got, want, (kind, fold, layer, "against numpy"))
        same_bits(model.pool(toks, layer, varlen=True), got, (kind, fold, layer, "varlen"))
        for b, n in enumerate(LENS):
            same_bits(model.pool(toks[b:b + 1, :n + 2].contiguous(), layer), got[b:b + 1], (kind, fold, layer, b, "alone"))
    empty = torch.tensor([[0, 2, 1, 1]]).cuda()  # <cls> <eos>: no residue, a zero vector
    assert not model.pool(empty, 1).any()


# ---- the index ------------------------------------------------------------------------------------------------------------
ALPHABET = esm.Alphabet.from_architecture("ESM-1b")


def records_of(n, seed, prefix, lo=4, hi=60):
    rng = np.random.default_rng(seed)
    return [(f"{prefix}{i}", "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=int(rng.integers(lo, hi))))) for i in range(n)]


def tolerance(ua, ub):
    """align's stated bound (tests/test_align_gpu.py): (S in fp64, max(8 err32, 2^-19 max|S|)), err32 the error of numpy's
    float32 matmul of the same fp32 rows"""
    S64 = ua.astype(np.float64) @ ub.astype(np.float64).T
    err32 = float(np.abs((ua @ ub.T).astype(np.float64) - S64).max())
    return S64, max(8 * err32, 2.0 ** -19 * float(np.abs(S64).max()))


@pytest.mark.parametrize("kind", ["esm2", "esm2_96", "esm1b"])
def test_index_build_file_and_search(kind, tmp_path, monkeypatch):
    model = in_mode(kind, True, monkeypatch)
    db, queries = records_of(14, 1, "t"), records_of(5, 2, "q")
    index = S.EmbeddingIndex.build(model, ALPHABET, db, layer=2, model_name="synth")
    assert index.meta == dict(layer=2, pooling="mean", num_layers=L, embed_dim=DIMS[kind][0], model="synth")
    assert index.labels == [r[0] for r in db] and index.sequences == [r[1] for r in db] and index.lengths.tolist() == [len(r[1]) for r in db]
    # the bits do not depend on the batching
    for kw in (dict(batch_tokens=70), dict(batch_tokens=300, varlen=False), dict(batch_tokens=10 ** 6, keep_sequences=False)):
        other = S.EmbeddingIndex.build(model, ALPHABET, db, layer=2, **kw)
        assert np.array_equal(ref.bits(other.vectors), ref.bits(index.vectors)), kw
    assert other.sequences is None
    convert = ALPHABET.get_batch_converter()
    one = model.pool(convert([db[3]])[2].cuda(), 2)
    assert np.array_equal(ref.bits(one.cpu().numpy()), ref.bits(index.vectors[3:4]))
    index.save(tmp_path / "db.npz")
    back = S.EmbeddingIndex.load(tmp_path / "db.npz").to("cuda")
    assert np.array_equal(ref.bits(back.vectors), ref.bits(index.vectors)) and back.meta == index.meta and back.sequences == index.sequences
    # search: against the numpy top-k of the similarity the GEMM wrote, and that against fp64
    qvec = S.pool_records(model, ALPHABET, queries, 2)
    out = back.search(qvec, 4, return_similarity=True)
    sim = out["similarity"].cpu().numpy()
    assert sim.shape == (5, 14)
    want_val, want_id = ref.topk_rows(sim, 4)
    assert np.array_equal(out["ids"].cpu().numpy(), want_id) and np.array_equal(ref.bits(out["scores"].cpu().numpy()), ref.bits(want_val))
    S64, tol = tolerance(aref.operand_rows(qvec.cpu().numpy(), "cosine"), aref.operand_rows(index.vectors, "cosine"))
    err = float(np.abs(sim.astype(np.float64) - S64).max())
    print(f"search accuracy: {kind}: |S - S64| = {err:.3g}, bound {tol:.3g}")
    assert err <= tol, (kind, err, tol)
    # model.search pools and searches; more hits than proteins end in unused slots
    toks = convert(queries)[2].cuda()
    via = model.search(back, toks, 20)
    assert torch.equal(via["ids"][:, :4], out["ids"]) and (via["ids"][:, 14:] == -1).all() and torch.isneginf(via["scores"][:, 14:]).all()
    assert (via["ids"][:, :14].sort(1).values == torch.arange(14, device="cuda", dtype=torch.int32)).all()
    # the index against itself
    own = back.search(back, 3, exclude_self=True, return_similarity=True)
    want_val, want_id = ref.topk_rows(own["similarity"].cpu().numpy(), 3, exclude=np.arange(14))
    assert np.array_equal(own["ids"].cpu().numpy(), want_id) and np.array_equal(ref.bits(own["scores"].cpu().numpy()), ref.bits(want_val))
    assert not (own["ids"].cpu().numpy() == np.arange(14)[:, None]).any()
    assert (back.search(back, 1)["ids"][:, 0].cpu().numpy() == np.arange(14)).all()


def test_one_block_equals_many():
    rng = np.random.default_rng(3)
    n, E, Q = 1000, 96, 7
    index = S.EmbeddingIndex(rng.standard_normal((n, E)).astype(np.float32), [str(i) for i in range(n)], np.ones(n)).to("cuda")
    q = torch.from_numpy(rng.standard_normal((Q, E)).astype(np.float32)).cuda()
    base = index.search(q, 50, return_similarity=True)
    want_val, want_id = ref.topk_rows(base["similarity"].cpu().numpy(), 50)
    assert np.array_equal(base["ids"].cpu().numpy(), want_id) and np.array_equal(ref.bits(base["scores"].cpu().numpy()), ref.bits(want_val))
    for max_bytes in (4 * Q * 512, 4 * Q * 256, 4 * 3 * 256, 4 * 256):  # 2 and 4 blocks; 3 and 7 chunks of queries
        qc, nb = S.plan_search(n, Q, max_bytes)
        assert (qc, nb) != S.plan_search(n, Q, 2 << 30)
        out = index.search(q, 50, max_bytes=max_bytes, return_similarity=True)
        for key in ("ids", "scores", "similarity"):
            same_bits(out[key], base[key], (max_bytes, key))
    ex = index.search(q, 50, exclude_self=True, max_bytes=4 * 3 * 256)
    want_val, want_id = ref.topk_rows(base["similarity"].cpu().numpy(), 50, exclude=np.arange(Q))
    assert np.array_equal(ex["ids"].cpu().numpy(), want_id) and np.array_equal(ref.bits(ex["scores"].cpu().numpy()), ref.bits(want_val))


# ---- prefilter + aligner --------------------------------------------------------------------------------------------------
def residues(model, records, layer):
    toks = ALPHABET.get_batch_converter()(records)[2].cuda()
    rep = model(toks, repr_layers=[layer])["representations"][layer]
    return [rep[k, 1:len(seq) + 1].contiguous() for k, (_, seq) in enumerate(records)]


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_search_and_align_is_the_aligner_on_the_hits(kind, monkeypatch):
    model = in_mode(kind, True, monkeypatch)
    db, queries = records_of(9, 4, "t", 8, 40), records_of(3, 5, "q", 8, 40)
    index = S.EmbeddingIndex.build(model, ALPHABET, db, layer=2).to("cuda")
    out = esm_amd.search_and_align(model, ALPHABET, queries, index, top_k=4, align_top=2, mode="local")
    ids = out["ids"].cpu().numpy()
    assert ids.shape == (3, 4)
    al = out["alignment"]
    assert al["pairs"].cpu().tolist() == [[q, int(ids[q, r])] for q in range(3) for r in range(2)]
    hand = esm_amd.align_embeddings(residues(model, queries, 2), residues(model, db, 2), pairs=al["pairs"].cpu(), mode="local")
    for key in ("score", "end", "start", "n_cols", "n_match", "col_offsets", "cols"):
        same_bits(al[key], hand[key], (kind, key))
    # groups of one query, scores only
    small = esm_amd.search_and_align(model, ALPHABET, queries, index, top_k=4, align_top=2, mode="local", batch_tokens=1, paths=False)
    assert "cols" not in small["alignment"]
    for key in ("pairs", "score", "end"):
        same_bits(small["alignment"][key], al[key], (kind, key, "groups"))
    same_bits(small["ids"], out["ids"])


# ---- the command line -----------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    from esm_amd import checkpoint

    model = in_mode("esm2", True, monkeypatch)
    other = model_of("esm2_96")
    models = {"synth": model, "other": other}
    monkeypatch.setattr(checkpoint, "load_model_and_alphabet", lambda location: (models[location], ALPHABET))
    db, queries = records_of(8, 6, "t", 8, 40), records_of(2, 7, "q", 8, 40)
    db[5] = ("t5", queries[0][1][2:] + "ACD")  # a relative of q0
    for name, records in (("db.fa", db), ("q.fa", queries)):
        (tmp_path / name).write_text("".join(f">{label} some description\n{seq}\n" for label, seq in records))
    npz, tsv, aln = str(tmp_path / "db.npz"), str(tmp_path / "hits.tsv"), str(tmp_path / "aln.txt")
    assert S.main(["index", "--model-location", "synth", "--fasta", str(tmp_path / "db.fa"), "--layer", "2", "--output", npz]) == 0
    index = S.EmbeddingIndex.load(npz)
    api = S.EmbeddingIndex.build(model, ALPHABET, db, layer=2)
    assert np.array_equal(ref.bits(index.vectors), ref.bits(api.vectors)) and index.labels == [r[0] for r in db]
    assert index.meta == dict(layer=2, pooling="mean", num_layers=L, embed_dim=128, model="synth") and index.sequences == [r[1] for r in db]
    base = ["query", "--model-location", "synth", "--index", npz, "--query", str(tmp_path / "q.fa"), "--top", "3", "--output", tsv]
    assert S.main(base) == 0
    hits = api.to("cuda").search(S.pool_records(model, ALPHABET, queries, 2), 3)
    ids, scores = hits["ids"].cpu().numpy(), hits["scores"].cpu().numpy()
    lines = [ln.split("\t") for ln in open(tsv).read().splitlines()]
    assert lines[0] == list(S.TSV_HEADER) and len(lines) == 7
    for q in range(2):
        for r in range(3):
            assert lines[1 + 3 * q + r] == [queries[q][0], db[ids[q, r]][0], str(r + 1), f"{scores[q, r]:.6f}"]
    assert lines[1][1] == "t5"
    # --align: the two best hits of every query, their lines end in align's columns
    assert S.main(base + ["--align", "--align-top", "2", "--mode", "local", "--alignments", aln]) == 0
    out = esm_amd.search_and_align(model, ALPHABET, queries, api, top_k=3, align_top=2, mode="local")["alignment"]
    lines = [ln.split("\t") for ln in open(tsv).read().splitlines()]
    assert lines[0] == list(S.TSV_HEADER) + list(esm_amd.align.TSV_HEADER[2:]) and len(lines) == 5
    score, nm = out["score"].cpu().numpy(), out["n_match"].cpu().numpy()
    start, end, off = out["start"].cpu().numpy(), out["end"].cpu().numpy(), out["col_offsets"].cpu().numpy()
    for p, (q, t) in enumerate(out["pairs"].cpu().tolist()):
        la, lb = len(queries[q][1]), len(db[t][1])
        rng_ = [f"{start[p][k] + 1}-{end[p][k]}" if end[p][k] > start[p][k] else "-" for k in (0, 1)]
        assert lines[1 + p] == [queries[q][0], db[t][0], str(p % 2 + 1), f"{scores[q, p % 2]:.6f}", f"{score[p]:.4f}",
                                f"{score[p] / min(la, lb):.4f}", str(nm[p]), rng_[0], rng_[1]], (p, lines[1 + p])
    text = open(aln).read().splitlines()
    assert len(text) == 12 and text[0].startswith(">q0 t5 score=")
    assert (text[1], text[2]) == esm_amd.alignment_strings(queries[0][1], db[5][1], out["cols"][off[0]:off[1]])
    # an index without sequences cannot be aligned; an index of another model is refused
    bare = str(tmp_path / "bare.npz")
    assert S.main(["index", "--model-location", "synth", "--fasta", str(tmp_path / "db.fa"), "--no-sequences", "--output", bare]) == 0
    assert S.EmbeddingIndex.load(bare).sequences is None and S.EmbeddingIndex.load(bare).meta["layer"] == L
    with pytest.raises(ValueError, match="--no-sequences"):
        S.main(base[:4] + [bare] + base[5:] + ["--align"])
    with pytest.raises(ValueError, match="embed_dim = 128, the model has embed_dim = 96"):
        S.main(["query", "--model-location", "other"] + base[3:])
    index.meta["layer"] = 7
    index.save(npz)
    with pytest.raises(ValueError, match="layer 7"):
        S.main(base)
