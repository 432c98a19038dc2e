"""What of esm_amd/search.py needs no GPU: the numpy top-k reference of tests/_search_ref.py against a brute force that does
not use its key, the block and group planners, the .npz handling, the TSV text and the argument refusals."""
import io
import itertools
import types

import numpy as np
import pytest
import torch

import _search_ref as ref
from esm_amd import search as S

PALETTE = [-np.inf, -2.5, -1.0, -0.0, 0.0, 1.0, 1.0, 2.5, np.inf, np.nan]


# ---- the reference against brute force ------------------------------------------------------------------------------------
def test_order_is_the_total_order_of_the_bits():
    v = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 3.0, np.inf], dtype=np.float32)
    o = ref.order(v).astype(np.int64)
    assert np.all(np.diff(o) > 0)


@pytest.mark.parametrize("seed", range(6))
def test_topk_reference_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    for n, k in itertools.product([1, 2, 5, 12], [1, 3, 14]):
        for trial in range(8):
            row = rng.choice(PALETTE, size=n).astype(np.float32)
            id_base = int(rng.integers(0, 50))
            exclude = [None, id_base + int(rng.integers(0, n)), id_base + n + 3, -1][trial % 4]
            run_val = run_id = None
            cands = [(float(v), id_base + j) for j, v in enumerate(row) if exclude is None or id_base + j != exclude]
            if trial >= 4:  # a running list with used and unused slots; its ids are disjoint from the block's
                run_val = rng.choice(PALETTE[:-1], size=k).astype(np.float32)
                run_id = (1000 + rng.permutation(k)).astype(np.int32)
                unused = rng.random(k) < 0.3
                run_val[unused], run_id[unused] = -np.inf, -1
                cands += [(float(v), int(i)) for v, i in zip(run_val, run_id) if i >= 0]
            val, ids = ref.topk_merge(row, k, id_base, exclude, run_val, run_id)
            want = ref.brute_force_topk(cands, k)
            assert ids.tolist() == [w[1] for w in want], (seed, n, k, trial, row, want)
            assert np.array_equal(ref.bits(val), ref.bits(np.array([w[0] for w in want], dtype=np.float32))), (seed, n, k, trial)


def test_topk_reference_rules_by_hand():
    row = np.array([1.0, np.nan, 1.0, -0.0, 0.0, -np.inf], dtype=np.float32)
    val, ids = ref.topk_merge(row, 7, id_base=10)
    assert ids.tolist() == [10, 12, 14, 13, 15, -1, -1]  # ties to the lower id, +0.0 before -0.0, -inf a value, NaN none
    assert np.signbit(val[3]) and not np.signbit(val[2]) and np.all(np.isneginf(val[4:]))
    val, ids = ref.topk_merge(np.full(4, np.nan, dtype=np.float32), 2)
    assert ids.tolist() == [-1, -1] and np.all(np.isneginf(val))
    val, ids = ref.topk_merge(row, 2, id_base=10, exclude=10)
    assert ids.tolist() == [12, 14]


def test_pool_reference():
    x = np.arange(24, dtype=np.float32).reshape(6, 4)
    out = ref.pool_rows(x, np.array([0, 2, 2, 99, -5]), np.array([0, 1, 1, 3, 5]))
    assert np.array_equal(out, np.stack([x[0], np.zeros(4), x[2], (x[5] + x[0]) / 2]).astype(np.float32))


# ---- planners -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_db,n_q,max_bytes", [(1, 1, 1 << 30), (2000, 5, 1 << 30), (2000, 5, 5 * 4 * 256), (2000, 5, 4 * 256),
                                                (1 << 20, 256, 2 << 30), (1 << 24, 1, 2 << 30), (1000, 7, 30000)])
def test_plan_search(n_db, n_q, max_bytes):
    qc, nb = S.plan_search(n_db, n_q, max_bytes)
    assert 1 <= qc <= n_q and nb >= 256 and nb % 256 == 0 and nb <= S.MAX_BLOCK
    assert 4 * qc * nb <= max_bytes and nb <= (n_db + 255) // 256 * 256
    # the budget is used: a larger block or more queries would not fit, or there is nothing more to take
    assert qc == n_q or 4 * (qc + 1) * 256 > max_bytes
    assert nb == min((n_db + 255) // 256 * 256, S.MAX_BLOCK) or 4 * qc * (nb + 256) > max_bytes


def test_plan_search_refusals():
    with pytest.raises(ValueError, match="max_bytes"):
        S.plan_search(10, 1, 1023)
    with pytest.raises(ValueError, match="at least one"):
        S.plan_search(0, 1, 1 << 20)


def test_plan_groups():
    qt, tt = [10, 10, 10, 10], np.array([5, 6, 7, 8, 100])
    hits = [[0, 1], [1, 2], [3], [4, 0]]
    assert S.plan_groups(qt, hits, tt, 10 ** 6) == [(0, 4)]
    # 10 + 11 = 21; + 10 + 7 = 38; query 2 would make 56 > 40; query 3 alone is over the budget and still a group
    assert S.plan_groups(qt, hits, tt, 40) == [(0, 2), (2, 3), (3, 4)]
    assert S.plan_groups(qt, hits, tt, 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert S.plan_groups([], [], tt, 10) == []


def test_batches_cover_every_record_once():
    records = [(str(i), "A" * n) for i, n in enumerate([5, 50, 7, 7, 30, 1])]
    for budget in (1, 60, 10 ** 6):
        batches = S._batches(records, budget)
        assert sorted(i for b in batches for i in b) == list(range(6))
        for b in batches:
            assert len(b) == 1 or (max(len(records[i][1]) for i in b) + 2) * len(b) <= budget


# ---- the index on the host ------------------------------------------------------------------------------------------------
def small_index(sequences=True):
    rng = np.random.default_rng(0)
    seqs = ["ACDE", "FGHIKL", "MN"]
    return S.EmbeddingIndex(rng.standard_normal((3, 8)).astype(np.float32), ["a", "b b", "ç"], [4, 6, 2], seqs if sequences else None,
                            dict(layer=2, num_layers=3, embed_dim=8, model="synth"))


@pytest.mark.parametrize("sequences", [True, False])
def test_npz_round_trip(tmp_path, sequences):
    index = small_index(sequences)
    path = tmp_path / "db.npz"
    index.save(path)
    with np.load(path, allow_pickle=False) as z:  # plain arrays only
        assert set(z.files) == {"vectors", "labels", "lengths", "meta"} | ({"sequences"} if sequences else set())
    back = S.EmbeddingIndex.load(path)
    assert np.array_equal(ref.bits(back.vectors), ref.bits(index.vectors)) and back.labels == index.labels
    assert back.lengths.tolist() == [4, 6, 2] and back.sequences == index.sequences and back.meta == index.meta
    assert back.meta["pooling"] == "mean" and len(back) == 3 and back.device is None


def test_a_pickled_file_is_refused(tmp_path):
    index = small_index()
    path = tmp_path / "bad.npz"
    np.savez(path, vectors=index.vectors, labels=np.array(index.labels, dtype=object), lengths=index.lengths, meta=np.array("{}"))
    with pytest.raises(ValueError, match="[Pp]ickle"):
        S.EmbeddingIndex.load(path)
    np.savez(tmp_path / "short.npz", vectors=index.vectors)
    with pytest.raises(ValueError, match="no array 'labels'"):
        S.EmbeddingIndex.load(tmp_path / "short.npz")


def test_index_refusals():
    v = np.zeros((3, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="3 vectors, 2 labels"):
        S.EmbeddingIndex(v, ["a", "b"], [1, 2, 3])
    with pytest.raises(ValueError, match="multiple of 4"):
        S.EmbeddingIndex(np.zeros((3, 6), dtype=np.float32), "abc", [1, 2, 3])
    with pytest.raises(ValueError, match="non-empty"):
        S.EmbeddingIndex(np.zeros((0, 8), dtype=np.float32), [], [])
    with pytest.raises(ValueError, match="pooling"):
        S.EmbeddingIndex(v, "abc", [1, 2, 3], meta=dict(pooling="max"))
    index = small_index()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.to("cpu")
    for bad, msg in ((0, "top_k must be"), (1025, "top_k must be")):
        with pytest.raises(ValueError, match=msg):
            index.search(torch.zeros(2, 8), bad)
    with pytest.raises(ValueError, match="E = 12"):
        index.search(torch.zeros(2, 12), 1)
    with pytest.raises(ValueError, match="queries must be"):
        index.search(torch.zeros(8), 1)
    with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
        index.search(torch.zeros(2, 8), 1)
    big = S.EmbeddingIndex(np.zeros((1 << 13, 4), dtype=np.float32), [""] * (1 << 13), [1] * (1 << 13))
    with pytest.raises(ValueError, match="return_similarity"):
        big.search(torch.zeros((1 << 11) + 1, 4), 1, return_similarity=True)
    assert small_index().image_bytes() == 256 * 3 * 64 * 2


def test_meta_mismatch_and_model_refusals():
    index = small_index()
    model = types.SimpleNamespace(num_layers=3, embed_dim=8)
    index.check_model(model)
    for other, msg in ((dict(num_layers=4, embed_dim=8), "num_layers = 3"), (dict(num_layers=3, embed_dim=16), "embed_dim = 8")):
        with pytest.raises(ValueError, match=msg):
            index.check_model(types.SimpleNamespace(**other))
    index.meta["layer"] = 5
    with pytest.raises(ValueError, match="layer 5"):
        index.check_model(model)
    with pytest.raises(ValueError, match="outside 0 .. 3"):
        S.check_model(model, 4)
    with pytest.raises(NotImplementedError, match="window"):
        S.check_model(model, 1, window=64)
    assert S.check_model(model, None) == 3
    with pytest.raises(ValueError, match="no sequences"):
        S.search_and_align(model, None, [("q", "ACD")], small_index(sequences=False), 2)


# ---- text -----------------------------------------------------------------------------------------------------------------
def test_tsv_text():
    hits = [dict(query="q1", target="t2", rank=1, cosine=0.98765432, score=3.25, la=10, lb=20, n_match=4, start=[1, 2], end=[5, 7]),
            dict(query="q1", target="t9", rank=2, cosine=-0.5, score=0.0, la=10, lb=5, n_match=0, start=[0, 0], end=[0, 0])]
    buf = io.StringIO()
    S.write_tsv(buf, hits)
    assert buf.getvalue() == "query\ttarget\trank\tcosine\nq1\tt2\t1\t0.987654\nq1\tt9\t2\t-0.500000\n"
    buf = io.StringIO()
    S.write_tsv(buf, hits, aligned=True)
    lines = buf.getvalue().splitlines()
    assert lines[0] == "query\ttarget\trank\tcosine\tscore\tscore_per_residue\tn_match\tquery_range\ttarget_range"
    assert lines[1] == "q1\tt2\t1\t0.987654\t3.2500\t0.3250\t4\t2-5\t3-7"
    assert lines[2] == "q1\tt9\t2\t-0.500000\t0.0000\t0.0000\t0\t-\t-"
    buf = io.StringIO()
    S.write_tsv(buf, [], aligned=True)
    assert buf.getvalue().splitlines() == [lines[0]]


# ---- command line arguments -------------------------------------------------------------------------------------------------
def test_command_line_refusals(tmp_path, capsys):
    q = ["query", "--model-location", "m", "--index", "db.npz", "--query", "q.fa", "--output", "o.tsv"]
    for extra in (["--top", "0"], ["--top", "1025"], [], ["--top", "5", "--align-top", "2"], ["--top", "5", "--alignments", "a.txt"],
                  ["--top", "5", "--enhance"], ["--top", "5", "--align", "--align-top", "0"], ["--top", "5", "--mode", "semi"]):
        with pytest.raises(SystemExit):
            S.parse_args(q + extra)
    with pytest.raises(SystemExit):
        S.parse_args(["index", "--model-location", "m", "--output", "db.npz"])
    with pytest.raises(SystemExit):
        S.parse_args([])
    capsys.readouterr()
    args = S.parse_args(q + ["--top", "5", "--align", "--align-top", "2", "--mode", "local"])
    assert args.command == "query" and args.align and args.align_top == 2 and args.max_bytes == 2 << 30
    # what main refuses before it loads a model: bad gap penalties, --align on an index without sequences
    small_index(sequences=False).save(tmp_path / "db.npz")
    base = ["query", "--model-location", "none", "--index", str(tmp_path / "db.npz"), "--query", "q.fa", "--output", "o.tsv", "--top", "2"]
    with pytest.raises(ValueError, match="gap_extend"):
        S.main(base + ["--align", "--gap-open", "0.1", "--gap-extend", "0.5"])
    with pytest.raises(ValueError, match="--no-sequences"):
        S.main(base + ["--align"])
