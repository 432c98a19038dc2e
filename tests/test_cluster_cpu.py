"""What of esm_amd/cluster.py and of the centred index needs no GPU: the sequential reference of tests/_cluster_ref.py against a
brute force that keeps a set of covered nodes and no CSR, the centre arithmetic against fp64, the ``center`` array in the file,
priorities (ties, NaN), the TSV text and every argument refusal of the Python layer and the parser."""
import io
import math

import numpy as np
import pytest
import torch

import _cluster_ref as cref
import _search_ref as ref
import esm_amd
from esm_amd import cluster as C
from esm_amd import search as S


# ---- the reference against brute force ------------------------------------------------------------------------------------
def brute_force(adj, score, priority, assign):
    """Greedy incremental clustering on a dense boolean adjacency ``adj[u][w]`` (u covers w) without a CSR: nodes sorted by
    (priority descending, id), a set of covered nodes, and per member a scan over all representatives."""
    n = len(priority)
    walk = sorted(range(n), key=lambda i: (-priority[i], i))
    pos = {u: r for r, u in enumerate(walk)}
    covered, reps = set(), []
    for u in walk:
        if u in covered:
            continue
        reps.append(u)
        covered.update(w for w in range(n) if adj[u][w] and w != u and w not in reps)
    rep_of = list(range(n))

    def total(v):  # the total order of the IEEE bits on floats without NaN: value, then -0.0 below +0.0
        return (v, math.copysign(1.0, v))

    for w in range(n):
        if w in reps:
            continue
        cands = [u for u in reps if pos[u] < pos[w] and adj[u][w]]
        assert cands, (w, reps)
        if assign == "first":
            rep_of[w] = min(cands, key=lambda u: pos[u])
        else:
            rep_of[w] = min(cands, key=lambda u: (tuple(-x for x in total(float(score[u][w]))), pos[u]))
    return rep_of, reps, [rep_of.count(u) for u in reps]


def csr(adj, score):
    n = len(adj)
    offsets, ids, scores = [0], [], []
    for u in range(n):
        for w in range(n):
            if adj[u][w] and w != u:
                ids.append(w)
                scores.append(score[u][w])
        offsets.append(len(ids))
    return np.array(offsets, dtype=np.int64), np.array(ids, dtype=np.int32), np.array(scores, dtype=np.float32)


@pytest.mark.parametrize("assign", ["first", "nearest"])
@pytest.mark.parametrize("seed", range(8))
def test_sequential_reference_against_brute_force(seed, assign):
    rng = np.random.default_rng(seed)
    for n in (1, 2, 5, 13, 30):
        for density in (0.0, 0.08, 0.3, 1.0):
            adj = rng.random((n, n)) < density  # directed: adj[u][w] says nothing about adj[w][u]
            score = rng.choice(np.array([0.5, 0.5, 0.75, -0.0, 0.0, 1.0, -1.0], dtype=np.float32), (n, n))  # equal scores abound
            priority = rng.integers(0, 4, n)  # ties abound
            want = brute_force(adj, score, priority.tolist(), assign)
            offsets, ids, scores = csr(adj, score)
            rank = cref.rank_of(priority)
            rep_of, reps, sizes = cref.greedy(offsets, ids, scores, rank, assign)
            assert rep_of.tolist() == want[0] and reps.tolist() == want[1] and sizes.tolist() == want[2], (seed, n, density)
            assert sizes.sum() == n and (rep_of[reps] == reps).all()


@pytest.mark.parametrize("seed", range(4))
def test_rounds_give_the_sequential_representatives(seed):
    """The restated rounds (mark, decide) choose the sequential loop's representatives on random directed graphs; a chain in
    rank order takes one round per node."""
    rng = np.random.default_rng(100 + seed)
    for n in (1, 2, 7, 40):
        for density in (0.0, 0.05, 0.3, 1.0):
            adj = rng.random((n, n)) < density
            offsets, ids, scores = csr(adj, np.ones((n, n), dtype=np.float32))
            rank = cref.rank_of(rng.integers(0, 5, n))
            is_rep, rounds = cref.rounds_of(offsets, ids, rank)
            reps = cref.greedy(offsets, ids, scores, rank)[1]
            assert sorted(np.nonzero(is_rep)[0].tolist()) == sorted(reps.tolist()) and 1 <= rounds <= n, (seed, n, density)
    n = 9
    chain = (np.minimum(np.arange(n + 1), n - 1), np.arange(1, n, dtype=np.int32))
    is_rep, rounds = cref.rounds_of(*chain, np.arange(n, dtype=np.int32))
    assert is_rep.tolist() == [True, False] * 4 + [True] and rounds == n


def test_reference_by_hand():
    # 0 -> 1 -> 2 (a chain in rank order), 3 -> 2 with a greater score, 4 alone
    offsets = np.array([0, 1, 2, 2, 3, 3])
    ids = np.array([1, 2, 2], dtype=np.int32)
    scores = np.array([0.9, 0.8, 0.95], dtype=np.float32)
    rank = cref.rank_of([5, 4, 1, 3, 2])
    assert rank.tolist() == [0, 1, 4, 2, 3]
    rep_of, reps, sizes = cref.greedy(offsets, ids, scores, rank)
    assert rep_of.tolist() == [0, 0, 3, 3, 4] and reps.tolist() == [0, 3, 4] and sizes.tolist() == [2, 2, 1]  # 1 is covered: it covers nobody
    # an asymmetric pair: 0 -> 1 only.  With 0 first it covers 1; with 1 first nothing covers anything
    pair = (np.array([0, 1, 1]), np.array([1], dtype=np.int32), np.array([0.7], dtype=np.float32))
    assert cref.greedy(*pair, cref.rank_of([2, 1]))[0].tolist() == [0, 0]
    assert cref.greedy(*pair, cref.rank_of([1, 2]))[0].tolist() == [0, 1]
    # nearest: two representatives list node 2; the second has the greater score; equal scores go to the lower rank
    offsets, ids = np.array([0, 1, 2, 2]), np.array([2, 2], dtype=np.int32)
    for sc, first, nearest in (([0.6, 0.8], 0, 1), ([0.8, 0.8], 0, 0), ([0.0, -0.0], 0, 0), ([-0.0, 0.0], 0, 1)):
        sc = np.array(sc, dtype=np.float32)
        assert cref.greedy(offsets, ids, sc, cref.rank_of([3, 2, 1]), "first")[0].tolist() == [0, 1, first]
        assert cref.greedy(offsets, ids, sc, cref.rank_of([3, 2, 1]), "nearest")[0].tolist() == [0, 1, nearest]


def test_range_reference_rules():
    row = np.array([[0.5, np.nan, 0.25, -0.0, 0.0, np.inf, -np.inf, 0.5000001]], dtype=np.float32)
    counts, ids, scores = cref.range_rows(row, 0.5, id_base=10)
    assert counts.tolist() == [3] and ids.tolist() == [10, 15, 17]  # a tie passes, NaN never
    assert cref.range_rows(row, 0.0)[1].tolist() == [0, 2, 3, 4, 5, 7]  # -0.0 >= +0.0
    assert cref.range_rows(row, -np.inf)[1].tolist() == [0, 2, 3, 4, 5, 6, 7]
    assert cref.range_rows(row, np.nan)[0].tolist() == [0]
    assert cref.range_rows(row, 0.5, id_base=10, exclude=[15])[1].tolist() == [10, 17]
    S2 = np.array([[1.0, 0.6, 0.1], [0.4, 1.0, 0.7], [np.nan, 0.7, 1.0]], dtype=np.float32)
    offsets, ids, scores = cref.csr_of(S2, 0.5, exclude_self=True)
    assert offsets.tolist() == [0, 1, 2, 3] and ids.tolist() == [1, 2, 1] and scores.tolist() == [np.float32(0.6), np.float32(0.7), np.float32(0.7)]
    counts, ids2, scores2 = cref.range_rows(S2, 0.5, exclude=[0, 1, 2])
    assert np.array_equal(np.cumsum(counts), offsets[1:]) and np.array_equal(ids, ids2) and np.array_equal(scores, scores2)


# ---- centring -------------------------------------------------------------------------------------------------------------
def small_index(center=False, sequences=True, n=37, E=8, seed=0):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n, E)) + 3 * rng.standard_normal(E)).astype(np.float32)
    seqs = ["A" * (3 + i % 5) for i in range(n)]
    index = S.EmbeddingIndex(v, [f"p{i}" for i in range(n)], [len(s) for s in seqs], seqs if sequences else None,
                             dict(layer=2, num_layers=3, embed_dim=E, model="synth"))
    return index.centered() if center else index


def test_centering_against_fp64():
    index = small_index()
    got = index.centered()
    center, vectors = cref.center_of(index.vectors)
    assert got.center.dtype == np.float32 and np.array_equal(ref.bits(got.center), ref.bits(center))
    assert np.array_equal(ref.bits(got.vectors), ref.bits(vectors))
    assert got.labels == index.labels and got.sequences == index.sequences and got.meta == index.meta and got.lengths.tolist() == index.lengths.tolist()
    assert index.center is None and got.device is None
    # against fp64: the centre is the correctly rounded mean up to the rounding of the fp64 sum, a centred entry one fp32 rounding away
    mean64 = index.vectors.astype(np.float64).mean(0)
    assert np.abs(got.center - mean64).max() <= 2.0 ** -24 * np.abs(mean64).max() * 1.001
    exact = index.vectors.astype(np.float64) - got.center.astype(np.float64)
    assert np.abs(got.vectors - exact).max() <= 2.0 ** -24 * np.abs(exact).max()
    # what is left of the mean: the centre's rounding plus the entries' roundings, each at most 2^-24 of the largest magnitude
    assert np.abs(got.vectors.astype(np.float64).mean(0)).max() <= 2.0 ** -23 * np.abs(index.vectors).max()
    with pytest.raises(ValueError, match="centred already"):
        got.centered()


def test_the_center_array_in_the_file(tmp_path):
    plain, centred = small_index(), small_index(center=True)
    plain.save(tmp_path / "plain.npz")
    centred.save(tmp_path / "centred.npz")
    with np.load(tmp_path / "plain.npz", allow_pickle=False) as z:
        assert set(z.files) == {"vectors", "labels", "lengths", "meta", "sequences"}  # an uncentred file: what it always held
    with np.load(tmp_path / "centred.npz", allow_pickle=False) as z:
        assert set(z.files) == {"vectors", "labels", "lengths", "meta", "sequences", "center"}
    assert S.EmbeddingIndex.load(tmp_path / "plain.npz").center is None
    back = S.EmbeddingIndex.load(tmp_path / "centred.npz")
    assert np.array_equal(ref.bits(back.center), ref.bits(centred.center)) and np.array_equal(ref.bits(back.vectors), ref.bits(centred.vectors))
    with pytest.raises(ValueError, match="center has 4 entries"):
        S.EmbeddingIndex(plain.vectors, plain.labels, plain.lengths, center=np.zeros(4))


def test_a_mismatching_center_is_refused():
    plain, centred = small_index(), small_index(center=True)
    other = small_index(center=True, seed=1)
    for db, q in ((centred, plain), (plain, centred), (centred, other)):
        for call in (lambda: db.search(q, 1), lambda: db.range_search(q, 0.5)):
            with pytest.raises(ValueError, match="do not hold the same center"):
                call()
    # the same centre, or none on both sides, passes this check (and stops at the missing device image)
    same = S.EmbeddingIndex(centred.vectors[:3], "abc", [1, 2, 3], center=centred.center.copy())
    for db, q in ((centred, same), (plain, plain)):
        with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
            db.range_search(q, 0.5)
        with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
            db.search(q, 1)


# ---- priorities -----------------------------------------------------------------------------------------------------------
def test_priority_ties_and_nan():
    for prio in ([3, 1, 3, 2, 1], [0.5, -0.0, 0.0, 0.5, np.inf], [7] * 6, np.arange(5)):
        want = cref.rank_of(prio)
        rank, order = C.rank_of(torch.as_tensor(np.asarray(prio)))
        assert rank.tolist() == want.tolist() and order.tolist() == np.argsort(want).tolist(), prio
    assert cref.rank_of([3, 1, 3, 2, 1]).tolist() == [0, 3, 1, 2, 4]
    with pytest.raises(ValueError, match="NaN"):
        C.check_args(0.5, np.array([1.0, np.nan]), n=2)
    with pytest.raises(ValueError, match="NaN"):
        cref.rank_of(np.array([1.0, np.nan]))
    assert C.check_args(0.5, [3, 1], n=2).dtype == np.int64 and C.check_args(0.5, torch.tensor([0.5, 1.0]), n=2).dtype == np.float64
    assert C.check_args(0.5, "degree") is None


def test_list_lanes():
    assert [C.list_lanes(nnz, 100) for nnz in (0, 100, 101, 300, 3100, 3300, 10 ** 6)] == [1, 1, 2, 4, 32, 64, 64]


# ---- text -----------------------------------------------------------------------------------------------------------------
def test_tsv_text():
    offsets = np.array([0, 2, 2, 3, 3])
    ids = np.array([1, 3, 1], dtype=np.int32)
    scores = np.array([0.75, 0.987654321, 0.5], dtype=np.float32)
    rep_of = np.array([0, 0, 2, 0], dtype=np.int32)
    cos = C.member_cosines(rep_of, offsets, ids, scores)
    assert cos.tolist() == [1.0, 0.75, 1.0, np.float32(0.987654321)]
    buf = io.StringIO()
    C.write_tsv(buf, ["a", "b b", "c", "d"], rep_of, cos, {0: 3, 2: 1})
    assert buf.getvalue() == ("member\trepresentative\tcosine\tcluster_size\n"
                              "a\ta\t1.000000\t3\nb b\ta\t0.750000\t3\nc\tc\t1.000000\t1\nd\ta\t0.987654\t3\n")
    with pytest.raises(ValueError, match="not in the out-list"):
        C.member_cosines(np.array([0, 0, 2, 2], dtype=np.int32), offsets, ids, scores)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    index = small_index(center=True)
    n = len(index)
    for kw, msg in ((dict(threshold=float("nan")), "threshold is NaN"), (dict(threshold=0.5, assign="best"), "assign must be"),
                    (dict(threshold=0.5, priority="size"), "priority must be"), (dict(threshold=0.5, priority=np.zeros(n + 1)), r"must be \[N\]"),
                    (dict(threshold=0.5, priority=np.zeros((n, 2))), r"must be \[N\]"), (dict(threshold=0.5, priority=np.array(["a"] * n)), "ints or floats"),
                    (dict(threshold=0.5, priority=np.full(n, np.nan)), "NaN")):
        with pytest.raises(ValueError, match=msg):
            index.cluster(**kw)
        with pytest.raises(ValueError, match=msg):
            esm_amd.cluster_embeddings(index, **kw)
    with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
        index.cluster(0.5)
    for bad, msg in ((dict(threshold=float("nan")), "threshold is NaN"), (dict(threshold=0.5, max_edges=-1), "max_edges"),
                     (dict(threshold=0.5, max_bytes=100), "max_bytes")):
        with pytest.raises(ValueError, match=msg):
            index.range_search(torch.zeros(2, 8), **bad)
    with pytest.raises(ValueError, match="E = 12"):
        index.range_search(torch.zeros(2, 12), 0.5)
    with pytest.raises(ValueError, match="queries must be"):
        index.range_search(torch.zeros(8), 0.5)
    with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
        index.range_search(torch.zeros(2, 8), 0.5)


def test_command_line_refusals(tmp_path, capsys):
    base = ["--index", "db.npz", "--output", "o.tsv"]
    for extra in ([], ["--threshold", "nan"], ["--threshold", "x"], ["--threshold", "0.5", "--priority", "size"],
                  ["--threshold", "0.5", "--assign", "best"], ["--threshold", "0.5", "--max-edges", "-1"]):
        with pytest.raises(SystemExit):
            C.parse_args(base + extra)
    with pytest.raises(SystemExit):
        C.parse_args(["--threshold", "0.5", "--output", "o.tsv"])
    with pytest.raises(SystemExit):
        C.parse_args(["--threshold", "0.5", "--index", "db.npz"])
    capsys.readouterr()
    args = C.parse_args(base + ["--threshold", "0.5", "--center", "--priority", "degree", "--assign", "nearest"])
    assert args.center and args.priority == "degree" and args.assign == "nearest" and args.max_edges == 1 << 28 and args.representatives is None
    # the search module's index command takes --center
    assert S.parse_args(["index", "--model-location", "m", "--fasta", "f", "--output", "o", "--center"]).center
    assert not S.parse_args(["index", "--model-location", "m", "--fasta", "f", "--output", "o"]).center
    # what main refuses before it touches a device
    small_index(sequences=False).save(tmp_path / "bare.npz")
    small_index(center=True).save(tmp_path / "centred.npz")
    with pytest.raises(ValueError, match="--no-sequences"):
        C.main(["--index", str(tmp_path / "bare.npz"), "--threshold", "0.5", "--output", "o.tsv", "--representatives", "r.fa"])
    with pytest.raises(ValueError, match="centred already"):
        C.main(["--index", str(tmp_path / "centred.npz"), "--threshold", "0.5", "--output", "o.tsv", "--center"])


def test_lazy_exports():
    assert esm_amd.cluster_embeddings is C.cluster_embeddings and esm_amd.cluster is C
