"""Range search, centring and clustering end to end (esm_amd/search.py, esm_amd/cluster.py) on a planted set of 12 families of
50 vectors at E = 128 with a large common component: the families come back exactly on the centred index and collapse into one
cluster on the raw one; ``range_search`` against the thresholded similarity matrix of ``search`` bit for bit, in one block and
in many; ``cluster`` against the sequential reference of tests/_cluster_ref.py on that matrix for every priority and assignment
rule; ``search`` on a centred index; the command line without a model; and one run through a synthetic ESM-2."""
import functools

import numpy as np
import pytest
import torch

import _align_ref as aref
import _cluster_ref as cref
import _search_ref as ref
import esm
import esm_amd
from esm_amd import cluster as C
from esm_amd import search as S
from esm_amd.synth import synth_esm2_state_dict

pytestmark = pytest.mark.gpu
E, FAMILIES, MEMBERS = 128, 12, 50
N_ALL = FAMILIES * MEMBERS
FAMILY = np.repeat(np.arange(FAMILIES), MEMBERS)
RESIDUES = "ACDEFGHIKLMNPQRSTVWY"


def cosines(x):
    u = x / np.linalg.norm(x, axis=1, keepdims=True)
    return u @ u.T


@functools.lru_cache(maxsize=None)
def planted():
    """(vectors fp64 [600, E], lengths, sequences): ``default_rng(0)``; a common component 3 * standard_normal(E), 12 family
    centres standard_normal, 50 members per family = centre + common + 0.25 * standard_normal."""
    rng = np.random.default_rng(0)
    common = 3 * rng.standard_normal(E)
    centres = rng.standard_normal((FAMILIES, E))
    v = (centres[:, None, :] + common + 0.25 * rng.standard_normal((FAMILIES, MEMBERS, E))).reshape(N_ALL, E)
    lengths = rng.integers(8, 40, N_ALL)
    sequences = ["".join(rng.choice(list(RESIDUES), size=int(n))) for n in lengths]
    return v, lengths, sequences


@functools.lru_cache(maxsize=None)
def indices():
    """(raw index, centred index) on the device, and per index the similarity matrix of the index against itself as the GEMM
    wrote it: the reference every test here shares."""
    v, lengths, sequences = planted()
    raw = S.EmbeddingIndex(v.astype(np.float32), [f"f{FAMILY[i]}_{i}" for i in range(N_ALL)], lengths, sequences,
                           dict(layer=2, num_layers=3, embed_dim=E, model="planted"))
    centred = raw.centered()
    raw.to("cuda"), centred.to("cuda")
    sims = tuple(ix.search(ix, 1, return_similarity=True)["similarity"].cpu().numpy() for ix in (raw, centred))
    return raw, centred, sims


def same_csr(got, want, what):
    for g, w, name in zip((got["offsets"], got["ids"], got["scores"]), want, ("offsets", "ids", "scores")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(ref.bits(g) if g.dtype == np.float32 else g, ref.bits(w) if w.dtype == np.float32 else w), (what, name)


def same_clusters(got, want, what):
    for g, w, name in zip((got["rep_of"], got["representatives"], got["sizes"]), want, ("rep_of", "representatives", "sizes")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:8], w[:8])


def test_the_planted_set_has_the_margins():
    v, _, _ = planted()
    same = FAMILY[:, None] == FAMILY[None, :]
    c, r = cosines(v - v.mean(0)), cosines(v)
    print(f"planted set: centred within >= {c[same].min():.6f}, between <= {c[~same].max():.6f}; raw >= {r.min():.6f}")
    # 0.863095, 0.202021 and 0.825964 in fp64: the figures 0.863, 0.202 and 0.826 at the three decimals they are stated with
    assert round(c[same].min(), 3) >= 0.863 and round(c[~same].max(), 3) <= 0.202 and round(r.min(), 3) >= 0.826
    assert c[same].min() - c[~same].max() > 0.66  # the margin the thresholds below stand in
    # ... and the fp32 index keeps them: centring is the reference's arithmetic, bit for bit
    raw, centred, _ = indices()
    center, vectors = cref.center_of(raw.vectors)
    assert np.array_equal(ref.bits(centred.center), ref.bits(center)) and np.array_equal(ref.bits(centred.vectors), ref.bits(vectors))


def test_families_come_back_centred_and_collapse_raw():
    raw, centred, _ = indices()
    for priority in ("length", "degree"):
        for assign in ("first", "nearest"):
            out = centred.cluster(0.5, priority=priority, assign=assign)
            rep_of = out["rep_of"].cpu().numpy()
            reps = out["representatives"].cpu().numpy()
            assert len(reps) == FAMILIES and sorted(FAMILY[reps].tolist()) == list(range(FAMILIES)), (priority, assign)
            assert np.array_equal(FAMILY[rep_of], FAMILY) and out["sizes"].cpu().tolist() == [MEMBERS] * FAMILIES  # exactly the families
            assert out["rounds"] == 2 and out["rank"].dtype == torch.int32 and out["rep_of"].dtype == torch.int32
            if priority == "length":  # the longest member (the lowest id among equals) represents its family
                for u in reps:
                    members = np.nonzero(FAMILY == FAMILY[u])[0]
                    assert u == members[np.argmax(centred.lengths[members])]
    out = raw.cluster(0.5)  # every raw cosine is above 0.8: the threshold separates nothing
    assert out["representatives"].numel() == 1 and out["sizes"].cpu().tolist() == [N_ALL] and (out["rep_of"] == out["representatives"][0]).all()
    assert esm_amd.cluster_embeddings(raw, 0.5)["rep_of"].equal(out["rep_of"])


@pytest.mark.parametrize("threshold", [0.5, 0.1, -0.05])
def test_range_search_is_the_thresholded_similarity(threshold):
    raw, centred, (_, sim) = indices()
    for exclude_self in (False, True):
        want = cref.csr_of(sim, threshold, exclude_self)
        one = centred.range_search(centred, threshold, exclude_self=exclude_self)
        same_csr(one, want, (threshold, exclude_self, "one block"))
        for max_bytes in (4 * N_ALL * 256, 4 * 100 * 256, 4 * 256):  # 3 blocks; 6 chunks of queries; one query row a time
            assert S.plan_search(N_ALL, N_ALL, max_bytes) != S.plan_search(N_ALL, N_ALL, 2 << 30)
            same_csr(centred.range_search(centred, threshold, exclude_self=exclude_self, max_bytes=max_bytes), want, (threshold, exclude_self, max_bytes))
    if threshold == 0.5:
        assert want[0][-1] == N_ALL * (MEMBERS - 1)  # the families' pairs and no other
    # fp32 queries: the centre is subtracted on the device, the same bits as numpy's
    q = torch.from_numpy(raw.vectors[37:160]).cuda()
    want = cref.csr_of(sim[37:160], threshold)
    same_csr(centred.range_search(q, threshold), want, (threshold, "tensor queries"))
    same_csr(centred.range_search(q.cpu(), threshold, max_bytes=4 * 7 * 256), want, (threshold, "tensor queries from the host, blocks"))
    empty = centred.range_search(q[:0], threshold)
    assert empty["offsets"].tolist() == [0] and empty["ids"].numel() == 0 and empty["scores"].numel() == 0
    nothing = centred.range_search(q, 2.0)
    assert not nothing["offsets"].any() and nothing["ids"].numel() == 0 and nothing["ids"].dtype == torch.int32


@pytest.mark.parametrize("threshold", [0.5, 0.1, -0.05])
def test_cluster_is_the_sequential_loop(threshold):
    """At 0.1 and -0.05 the graph reaches across families and S[u][w] >= tau does not imply S[w][u] >= tau bit for bit: the
    reference reads the same directed matrix."""
    raw, centred, (_, sim) = indices()
    offsets, ids, scores = cref.csr_of(sim, threshold, exclude_self=True)
    rng = np.random.default_rng(1)
    priorities = {"length": centred.lengths, "degree": np.diff(offsets), "ints with ties": rng.integers(0, 5, N_ALL),
                  "floats": rng.standard_normal(N_ALL).astype(np.float32)}
    base = {}
    for name, prio in priorities.items():
        rank = cref.rank_of(prio)
        rounds = cref.rounds_of(offsets, ids, rank)[1]
        for assign in ("first", "nearest"):
            want = cref.greedy(offsets, ids, scores, rank, assign)
            arg = name if name in ("length", "degree") else (torch.from_numpy(prio) if name == "floats" else prio)
            out = centred.cluster(threshold, priority=arg, assign=assign)
            same_clusters(out, want, (threshold, name, assign))
            assert np.array_equal(out["rank"].cpu().numpy(), rank) and out["rounds"] == rounds, (threshold, name, assign, out["rounds"], rounds)
            same_csr(out["neighbors"], (offsets, ids, scores), (threshold, name, "neighbors"))
            base[name, assign] = out
    # the same result whatever the blocks
    for max_bytes in (4 * 100 * 256, 4 * 256):
        for (name, assign), want in base.items():
            if name in ("length", "degree"):
                out = centred.cluster(threshold, priority=name, assign=assign, max_bytes=max_bytes)
                for key in ("rep_of", "representatives", "sizes", "rank"):
                    assert torch.equal(out[key], want[key]), (threshold, name, assign, max_bytes, key)
                assert out["rounds"] == want["rounds"]


def test_max_edges():
    raw, centred, (raw_sim, _) = indices()
    assert (raw_sim >= 0.5).all()
    with pytest.raises(ValueError, match=r"threshold 0\.5 passes 359400 pairs, more than max_edges = 1000.*centered\(\)"):
        raw.cluster(0.5, max_edges=1000)
    with pytest.raises(ValueError, match=r"max_edges = 29399.*centered\(\)"):
        centred.range_search(centred, 0.5, exclude_self=True, max_edges=N_ALL * (MEMBERS - 1) - 1)
    assert centred.range_search(centred, 0.5, exclude_self=True, max_edges=N_ALL * (MEMBERS - 1))["ids"].numel() == N_ALL * (MEMBERS - 1)


def test_search_on_a_centred_index():
    raw, centred, (_, sim) = indices()
    k = 60
    q_raw = torch.from_numpy(raw.vectors[:90]).cuda()
    out = centred.search(q_raw, k, return_similarity=True)  # the centre is subtracted inside
    got_sim = out["similarity"].cpu().numpy()
    assert np.array_equal(ref.bits(got_sim), ref.bits(sim[:90]))  # the same bits as the host-centred vectors give
    want_val, want_id = ref.topk_rows(got_sim, k)
    assert np.array_equal(out["ids"].cpu().numpy(), want_id) and np.array_equal(ref.bits(out["scores"].cpu().numpy()), ref.bits(want_val))
    via_index = centred.search(centred, k)
    assert torch.equal(via_index["ids"][:90], out["ids"]) and torch.equal(via_index["scores"][:90], out["scores"])
    # against numpy on the centred vectors in fp64: the k best cosines, up to the product's error (bound of tests/test_search_gpu.py)
    _, vectors = cref.center_of(raw.vectors)
    u = aref.operand_rows(vectors, "cosine")
    S64 = u.astype(np.float64) @ u.astype(np.float64).T
    err32 = float(np.abs((u @ u.T).astype(np.float64) - S64).max())
    tol = max(8 * err32, 2.0 ** -19 * float(np.abs(S64).max()))
    err = float(np.abs(sim.astype(np.float64) - S64).max())
    print(f"centred search accuracy: |S - S64| = {err:.3g}, bound {tol:.3g}")
    assert err <= tol
    best64 = -np.sort(-S64[:90], axis=1)[:, :k]
    ids = out["ids"].cpu().numpy()
    # (two hits the device ranks the other way round lie within twice the error of each other)
    assert np.abs(np.take_along_axis(S64[:90], ids.astype(np.int64), 1) - best64).max() <= 2 * tol
    assert (FAMILY[ids[:, :MEMBERS]] == FAMILY[:90, None]).all() and (ids[:, 0] == np.arange(90)).all()  # the family first, oneself at its head
    # the raw index ranks by the common component: its scores are all high
    assert raw.search(q_raw, k)["scores"].min() > 0.8 and out["scores"][:, MEMBERS:].max() < 0.25


def test_command_line(tmp_path, monkeypatch):
    from esm_amd import checkpoint

    def no_model(*a, **k):
        raise AssertionError("the cluster command loads no model")

    monkeypatch.setattr(checkpoint, "load_model_and_alphabet", no_model)
    raw, centred, _ = indices()
    v, lengths, sequences = planted()
    plain = S.EmbeddingIndex(raw.vectors, raw.labels, raw.lengths, raw.sequences, raw.meta)
    npz, tsv, fasta = str(tmp_path / "db.npz"), str(tmp_path / "clusters.tsv"), str(tmp_path / "reps.fa")
    plain.save(npz)
    assert C.main(["--index", npz, "--threshold", "0.5", "--center", "--assign", "nearest", "--output", tsv, "--representatives", fasta]) == 0
    out = centred.cluster(0.5, assign="nearest")
    rep_of, reps, sizes = (out[k].cpu().numpy() for k in ("rep_of", "representatives", "sizes"))
    G = {k: t.cpu().numpy() for k, t in out["neighbors"].items()}
    lines = [ln.split("\t") for ln in open(tsv).read().splitlines()]
    assert lines[0] == list(C.TSV_HEADER) and len(lines) == 1 + N_ALL
    for w in range(N_ALL):
        u = rep_of[w]
        lo, hi = G["offsets"][u], G["offsets"][u + 1]
        cos = 1.0 if u == w else float(G["scores"][lo:hi][G["ids"][lo:hi] == w][0])
        assert lines[1 + w] == [raw.labels[w], raw.labels[u], f"{cos:.6f}", str(MEMBERS)], (w, lines[1 + w])
    text = open(fasta).read().splitlines()
    assert text == [x for u in reps for x in (">" + raw.labels[u], sequences[u])]
    # an index saved centred needs no --center, and gives the same file; the degree priority goes through
    centred_npz, tsv2 = str(tmp_path / "centred.npz"), str(tmp_path / "clusters2.tsv")
    S.EmbeddingIndex(centred.vectors, centred.labels, centred.lengths, None, centred.meta, centred.center).save(centred_npz)
    assert C.main(["--index", centred_npz, "--threshold", "0.5", "--assign", "nearest", "--output", tsv2]) == 0
    assert open(tsv2).read() == open(tsv).read()
    assert C.main(["--index", centred_npz, "--threshold", "0.5", "--priority", "degree", "--output", tsv2, "--max-bytes", str(4 * 256 * 64)]) == 0
    assert len(open(tsv2).read().splitlines()) == 1 + N_ALL
    with pytest.raises(ValueError, match="max_edges = 10"):
        C.main(["--index", npz, "--threshold", "0.5", "--output", tsv2, "--max-edges", "10"])
    with pytest.raises(ValueError, match="--no-sequences"):
        C.main(["--index", centred_npz, "--threshold", "0.5", "--output", tsv2, "--representatives", fasta])


def test_through_a_synthetic_esm2():
    """``EmbeddingIndex.build(...).centered().to(...).cluster(...)`` on ESM-2 (L = 3, E = 128): 30 random proteins and three
    variants of each of the first five, against the reference on the similarity matrix of the same index."""
    L, H = 3, 2
    model = esm.ESM2(L, E, H).eval()
    model.load_state_dict(synth_esm2_state_dict(L, E, H, seed=11), strict=True)
    model = model.cuda()
    alphabet = esm.Alphabet.from_architecture("ESM-1b")
    rng = np.random.default_rng(8)
    records = [(f"p{i}", "".join(rng.choice(list(RESIDUES), size=int(rng.integers(20, 60))))) for i in range(30)]
    for i in range(5):
        for j in range(3):
            seq = list(records[i][1])
            for pos in rng.integers(0, len(seq), 2):
                seq[pos] = RESIDUES[int(rng.integers(0, 20))]
            records.append((f"p{i}v{j}", "".join(seq) + "A" * j))
    built = S.EmbeddingIndex.build(model, alphabet, records, layer=2, model_name="synth")
    index = built.centered().to("cuda")
    center, vectors = cref.center_of(built.vectors)
    assert np.array_equal(ref.bits(index.center), ref.bits(center)) and np.array_equal(ref.bits(index.vectors), ref.bits(vectors))
    sim = index.search(index, 1, return_similarity=True)["similarity"].cpu().numpy()
    off_diag = sim[~np.eye(len(records), dtype=bool)]
    for threshold in (float(np.quantile(off_diag, 0.9)), 0.0):
        offsets, ids, scores = cref.csr_of(sim, threshold, exclude_self=True)
        for priority, prio in (("length", index.lengths), ("degree", np.diff(offsets))):
            for assign in ("first", "nearest"):
                out = index.cluster(threshold, priority=priority, assign=assign)
                rank = cref.rank_of(prio)
                same_clusters(out, cref.greedy(offsets, ids, scores, rank, assign), (threshold, priority, assign))
                same_csr(out["neighbors"], (offsets, ids, scores), (threshold, "neighbors"))
                assert out["rounds"] == cref.rounds_of(offsets, ids, rank)[1]
    # model.search on the centred index: the pooled queries lose the centre inside
    toks = alphabet.get_batch_converter()(records[:4])[2].cuda()
    hits = model.search(index, toks, 3)
    assert (hits["ids"][:, 0].cpu().numpy() == np.arange(4)).all() and (hits["scores"][:, 0] > 0.999).all()
