"""``model.align`` (esm_amd/align.py) through the synthetic models of esm_amd/synth.py — ESM-2 with L = 3 and E = 128 or E = 96
(Ep = 128: pad columns in the operand images), in both LayerNorm-fold settings, and one ESM-1b: against the numpy DP on the
returned similarity (bit for bit), the similarity against fp64, the equalities of bits between the ways to ask for the same
pair, self-alignment, and the command line."""
import argparse
import functools

import numpy as np
import pytest
import torch

import _align_ref as ref
import esm
import esm_amd
from esm_amd import align as A
from esm_amd.synth import synth_esm1b_state_dict, synth_esm2_state_dict, synth_tokens

pytestmark = pytest.mark.gpu
L = 3
DIMS = {"esm2": (128, 2), "esm2_96": (96, 6), "esm1b": (128, 2)}
FOLD = pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
LEN_A, LEN_B = [39, 17, 30], [25, 39, 8, 33]


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
    model(tokens_of(LEN_A, 3).cuda())
    assert model.ln_fold_active() is fold
    return model


def sides():
    return tokens_of(LEN_A, 3).cuda(), tokens_of(LEN_B, 4).cuda()


def same(a, b, keys=("score", "end", "start", "n_cols", "n_match", "col_offsets", "cols"), what=""):
    for key in keys:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key)
        assert torch.equal(a[key], b[key]), (what, key)


def pick(out, idx):
    """the listed pairs of a result, as a result of their own"""
    off = out["col_offsets"].cpu().numpy()
    cols = torch.cat([out["cols"][off[p]:off[p + 1]] for p in idx])
    nc = out["n_cols"][idx].long()
    sub = {k: out[k][idx] for k in ("score", "end", "start", "n_cols", "n_match")}
    sub.update(cols=cols, col_offsets=torch.cat([nc.new_zeros(1), nc.cumsum(0)]))
    return sub


def residues(model, toks, layer=L):
    """fp32 [L_k, E] per sequence, from the forward the caller would run"""
    rep = model(toks, repr_layers=[layer])["representations"][layer].float().cpu().numpy()
    t = toks.cpu().numpy()
    return [rep[k][(t[k] != 0) & (t[k] != 1) & (t[k] != 2)] for k in range(len(t))]


# ---- against the numpy DP on the returned similarity --------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", list(DIMS))
def test_against_the_numpy_dp(kind, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    ta, tb = sides()
    for mode, enhance in (("global", False), ("local", False), ("local", True), ("global", True)):
        out = model.align(ta, tb, mode=mode, enhance=enhance, return_similarity=True)
        assert out["pairs"].cpu().tolist() == [[a, b] for a in range(3) for b in range(4)]
        off = out["col_offsets"].cpu().numpy()
        host = {k: out[k].cpu().numpy() for k in ("score", "end", "start", "n_cols", "n_match", "cols")}
        for p, (a, b) in enumerate(out["pairs"].cpu().tolist()):
            S = out["similarity"][p].cpu().numpy()
            assert S.shape == (LEN_A[a], LEN_B[b])
            want = ref.align(S, mode, 1.0, 0.1)
            what = (kind, fold, mode, enhance, a, b)
            assert host["score"][p:p + 1].view(np.uint32)[0] == np.float32(want["score"]).reshape(1).view(np.uint32)[0], what
            assert tuple(host["end"][p]) == want["end"] and tuple(host["start"][p]) == want["start"], what
            assert np.array_equal(host["cols"][off[p]:off[p + 1]], want["cols"]) and host["n_match"][p] == want["n_match"], what
            assert host["n_cols"][p] == len(want["cols"]) == off[p + 1] - off[p], what


# ---- the similarity against fp64 ----------------------------------------------------------------------------------------
def tolerance(ua, ub):
    """(S in fp64, max(8 err32, 2^-19 max|S|), err32): err32 is the error of numpy's float32 matmul of the same fp32 rows.  The
    f16x3 product drops the lo lo term, loses bits of lo parts below 2^-14 and sums in another order than numpy; a numpy
    simulation of the split gave 1.1 - 3 x err32 at E = 320 .. 2560."""
    S64 = ua.astype(np.float64) @ ub.astype(np.float64).T
    err32 = float(np.abs((ua @ ub.T).astype(np.float64) - S64).max())
    return S64, max(8 * err32, 2.0 ** -19 * float(np.abs(S64).max())), err32


@FOLD
@pytest.mark.parametrize("similarity", ["cosine", "dot"])
@pytest.mark.parametrize("kind", list(DIMS))
def test_similarity_against_fp64(kind, similarity, fold, monkeypatch):
    model = in_mode(kind, fold, monkeypatch)
    ta, tb = sides()
    out = model.align(ta, tb, similarity=similarity, paths=False, return_similarity=True)
    assert "cols" not in out and "start" not in out
    ra, rb = residues(model, ta), residues(model, tb)
    worst = 0.0
    for p, (a, b) in enumerate(out["pairs"].cpu().tolist()):
        ua, ub = ref.operand_rows(ra[a], similarity), ref.operand_rows(rb[b], similarity)
        S64, tol, err32 = tolerance(ua, ub)
        err = float(np.abs(out["similarity"][p].cpu().numpy().astype(np.float64) - S64).max())
        worst = max(worst, err / err32)
        assert err <= tol, (kind, similarity, fold, a, b, err, tol, err32)
    print(f"align accuracy: {kind} {similarity} {'fold' if fold else 'plain'}: worst |S - S64| / err32 over 12 pairs = {worst:.2f}")


# ---- equalities of bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["global", "local"])
@pytest.mark.parametrize("kind", ["esm2", "esm2_96", "esm1b"])
def test_the_ways_to_ask_agree(kind, mode, monkeypatch):
    model = in_mode(kind, True, monkeypatch)
    ta, tb = sides()
    base = model.align(ta, tb, mode=mode)
    every = [(a, b) for a in range(3) for b in range(4)]
    same(base, model.align(ta, tb, mode=mode, pairs=every), what="explicit list")
    same(base, model.align(ta, tb, mode=mode, pairs=torch.tensor(every)), what="explicit tensor")
    # several blocks: the budget holds a little more than half of the whole (the largest single pair needs about 0.4 of it)
    E = DIMS[kind][0]
    budget = int(0.55 * A.block_bytes(LEN_A, LEN_B, every, E))
    assert len(A.plan_blocks(LEN_A, LEN_B, every, E, budget)) >= 3
    same(base, model.align(ta, tb, mode=mode, max_bytes=budget), what="blocks")
    # a pair inside the set, in a sparse list, and alone (its own token batches)
    some = [5, 2, 10]
    listed = model.align(ta, tb, mode=mode, pairs=[every[p] for p in some])
    same(pick(base, some), listed, what="sparse list")
    a, b = every[5]
    alone = model.align(ta[a:a + 1, :LEN_A[a] + 2].contiguous(), tb[b:b + 1, :LEN_B[b] + 2].contiguous(), mode=mode)
    same(pick(base, [5]), alone, what="alone")
    scores = model.align(ta, tb, mode=mode, paths=False)
    same(base, scores, keys=("score", "end"), what="scores only")


@pytest.mark.parametrize("kind", ["esm2", "esm1b"])
def test_varlen_is_the_padded_call(kind, monkeypatch):
    model = in_mode(kind, True, monkeypatch)
    ta, tb = sides()
    same(model.align(ta, tb, mode="local"), model.align(ta, tb, mode="local", varlen=True), what="varlen")


def test_align_embeddings_on_held_representations(monkeypatch):
    model = in_mode("esm2", True, monkeypatch)
    ta, tb = sides()
    base = model.align(ta, tb)
    ra = [torch.from_numpy(r).cuda() for r in residues(model, ta)]
    rb = [torch.from_numpy(r).cuda() for r in residues(model, tb)]
    same(base, esm_amd.align_embeddings(ra, rb), what="lists")
    same(base, esm_amd.align_embeddings((torch.cat(ra), LEN_A), (torch.cat(rb), torch.tensor(LEN_B))), what="flat")


# ---- self-alignment -------------------------------------------------------------------------------------------------------
@FOLD
@pytest.mark.parametrize("kind", list(DIMS))
def test_self_alignment_is_the_identity(kind, fold, monkeypatch):
    """Global, cosine: every diagonal cell is within the similarity tolerance ``tol`` of 1 and the path is the identity, so the
    score — the fp32 sum of the n diagonal cells in order — is within n tol + n^2 2^-24 (1 + tol) of n: n cells off by at most
    tol each, and n additions that each round a partial sum of at most n (1 + tol) to fp32."""
    model = in_mode(kind, fold, monkeypatch)
    ta, _ = sides()
    out = model.align(ta, ta, pairs=[(k, k) for k in range(3)])
    ra = residues(model, ta)
    off = out["col_offsets"].cpu().tolist()
    for k, n in enumerate(LEN_A):
        cols = out["cols"][off[k]:off[k + 1]].cpu().numpy()
        assert np.array_equal(cols, np.stack([np.arange(n), np.arange(n)], 1))
        assert int(out["n_match"][k]) == n and out["end"][k].tolist() == [n, n] and out["start"][k].tolist() == [0, 0]
        u = ref.operand_rows(ra[k], "cosine")
        _, tol, _ = tolerance(u, u)
        assert abs(float(out["score"][k]) - n) <= n * tol + n * n * 2.0 ** -24 * (1 + tol), (kind, fold, k, float(out["score"][k]), tol)


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    from esm_amd import checkpoint

    model = in_mode("esm2", True, monkeypatch)
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    monkeypatch.setattr(checkpoint, "load_model_and_alphabet", lambda location: (model, alphabet))
    rng = np.random.default_rng(8)
    draw = lambda n: "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=n))
    queries = [("q1", draw(21)), ("q2", draw(34))]
    targets = [("t1", draw(30)), ("t2", queries[0][1][3:18] + draw(9)), ("t3", draw(12))]
    for name, records in (("q.fa", queries), ("t.fa", targets)):
        (tmp_path / name).write_text("".join(f">{label} some description\n{seq}\n" for label, seq in records))
    convert = alphabet.get_batch_converter()
    ta, tb = convert(queries)[2].cuda(), convert(targets)[2].cuda()
    api = model.align(ta, tb, mode="local")
    base = ["--model-location", "synth", "--query", str(tmp_path / "q.fa"), "--target", str(tmp_path / "t.fa"), "--mode", "local"]
    assert A.main(base + ["--output", str(tmp_path / "hits.tsv"), "--alignments", str(tmp_path / "aln.txt")]) == 0
    lines = [ln.split("\t") for ln in (tmp_path / "hits.tsv").read_text().splitlines()]
    assert lines[0] == list(A.TSV_HEADER) and len(lines) == 7
    score, nm = api["score"].cpu().numpy(), api["n_match"].cpu().numpy()
    start, end = api["start"].cpu().numpy(), api["end"].cpu().numpy()
    off = api["col_offsets"].cpu().numpy()

    def line_of(p, q, t):
        la, lb = len(queries[q][1]), len(targets[t][1])
        rng_ = [f"{start[p][k] + 1}-{end[p][k]}" if end[p][k] > start[p][k] else "-" for k in (0, 1)]
        return [queries[q][0], targets[t][0], f"{score[p]:.4f}", f"{score[p] / min(la, lb):.4f}", str(nm[p]), rng_[0], rng_[1]]

    for p, (q, t) in enumerate((q, t) for q in range(2) for t in range(3)):
        assert lines[1 + p] == line_of(p, q, t), (p, lines[1 + p])
    text = (tmp_path / "aln.txt").read_text().splitlines()
    assert len(text) == 18 and text[0].startswith(">q1 t1 score=")
    want = A.alignment_strings(queries[0][1], targets[1][1], api["cols"][off[1]:off[2]])
    assert (text[4], text[5]) == want and want[0].replace("-", "") in queries[0][1]
    # --top 1: every pair is scored, exactly one target per query is traced and listed
    assert A.main(base + ["--output", str(tmp_path / "top.tsv"), "--top", "1"]) == 0
    top = [ln.split("\t") for ln in (tmp_path / "top.tsv").read_text().splitlines()][1:]
    assert len(top) == 2
    for q in range(2):
        t = int(np.argmax(score[3 * q:3 * q + 3]))
        assert top[q] == line_of(3 * q + t, q, t)
