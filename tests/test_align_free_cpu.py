"""Free end gaps and several hits per pair without a GPU: the numpy reference (tests/_align_free_ref.py) against a brute-force
enumeration of every path a mask allows, the arguments and their refusals, the new ABI entries' refusals before any HIP call,
and the command lines."""
import io

import numpy as np
import pytest
import torch

import _align_free_ref as fr
import _align_ref as ref
import esm
import esm_amd
from esm_amd import _native as N
from esm_amd import align as A
from esm_amd import msa_build as MB
from esm_amd import search as SE


def exact_S(rng, La, Lb, integer):
    """values whose sums are exact in fp32 and fp64 alike: integers in -2 .. 2 (many ties), or multiples of 1 / 4 in [-2, 2]"""
    if integer:
        return rng.integers(-2, 3, size=(La, Lb)).astype(np.float32)
    return (rng.integers(-8, 9, size=(La, Lb)) / 4.0).astype(np.float32)


# ---- the reference itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integer", [False, True], ids=["quarters", "integer"])
@pytest.mark.parametrize("o,e", [(1.0, 0.125), (0.5, 0.0)])
def test_reference_is_the_brute_force_optimum_for_every_mask(integer, o, e):
    rng = np.random.default_rng(11 + int(integer))
    for La in range(1, 6):
        for Lb in range(1, 6):
            S = exact_S(rng, La, Lb, integer)
            for mask in range(16):
                got = fr.align(S, "global", o, e, mask)
                assert float(got["score"]) == fr.brute_force(S, o, e, mask), (La, Lb, mask, S)
                cols, (i0, j0), (i1, j1) = got["cols"], got["start"], got["end"]
                assert ref.rescore(S, cols, o, e) == float(got["score"])
                # the path covers start .. end on both sides; a start off the corner needs its bit, and so does an end
                assert [i for i in cols[:, 0] if i >= 0] == list(range(i0, i1)) and [j for j in cols[:, 1] if j >= 0] == list(range(j0, j1))
                assert i0 == 0 or (j0 == 0 and mask & fr.A_START)
                assert j0 == 0 or (i0 == 0 and mask & fr.B_START)
                assert i1 >= 1 and j1 >= 1 and (i1 == La or (j1 == Lb and mask & fr.A_END)) and (j1 == Lb or (i1 == La and mask & fr.B_END))
                # the end cell: the first of the largest candidates, rows first
                H = got["H"]
                cand = fr.end_candidates(La, Lb, mask)
                assert (i1, j1) == min((c for c in cand if H[c] == max(H[c] for c in cand)))
                # the walk needs no border byte: the full-grid walk of the plain reference reads them and agrees
                w = ref.walk(got["tb_full"], got["end"], "global")
                assert np.array_equal(w[0], cols) and w[2] == got["start"]


def test_mask_zero_is_the_plain_reference():
    rng = np.random.default_rng(3)
    for La, Lb in [(1, 1), (3, 7), (12, 9), (20, 20)]:
        S = rng.uniform(-1, 1, size=(La, Lb)).astype(np.float32)
        for mode in ("global", "local"):
            a, b = ref.align(S, mode, 1.0, 0.1), fr.align(S, mode, 1.0, 0.1, 0)
            assert np.float32(a["score"]).tobytes() == np.float32(b["score"]).tobytes() and a["end"] == b["end"] and a["start"] == b["start"]
            assert np.array_equal(a["tb"], b["tb"]) and np.array_equal(a["cols"], b["cols"]) and np.array_equal(a["H"], b["H"])


def test_reference_hits_are_disjoint_and_non_increasing():
    rng = np.random.default_rng(4)
    for mode, mask in (("local", 0), ("global", 12), ("global", 15)):
        S = exact_S(rng, 9, 14, False)
        hits, after = fr.hits(S, 4, mode, 1.0, 0.25, mask)
        seen = set()
        for k, h in enumerate(hits):
            assert not np.isnan(h["H"]).any()
            assert k == 0 or float(h["score"]) <= float(hits[k - 1]["score"])
            cells = {(int(i), int(j)) for i, j in h["cols"] if i >= 0 and j >= 0}
            assert not cells & seen
            if k < 3:
                seen |= cells
        assert {(int(i), int(j)) for i, j in np.argwhere(np.isneginf(after))} == seen
    one, _ = fr.hits(np.ones((1, 1), dtype=np.float32), 3, "local")
    assert [h["n_match"] for h in one] == [1, 0, 0] and [float(h["score"]) for h in one] == [1.0, 0.0, 0.0]


# ---- arguments ----------------------------------------------------------------------------------------------------------
def test_free_ends_parsing():
    assert A.MODES == {"global": 0, "local": 1}
    assert [A.parse_free_ends(v) for v in (None, "a", "b", "both", 0, 7, 15, np.int64(9))] == [0, 3, 12, 15, 0, 7, 15, 9]
    assert A.parse_free_ends(["a_start", "b_end"]) == 9 and A.parse_free_ends(("b_start",)) == 4 and A.parse_free_ends("a_end") == 2
    assert A.parse_free_ends({"a_start", "a_end", "b_start", "b_end"}) == 15 and A.parse_free_ends([]) == 0
    for bad in (16, -1, "c", ["a"], ["a_start", 3], 1.0, True):
        with pytest.raises(ValueError, match="free_ends"):
            A.parse_free_ends(bad)
    assert A.check_hits("global", "b", 3, 0.5) == (12, 3, 0.5) and A.check_hits("local", None, 16) == (0, 16, 0.0)


def test_argument_errors_come_before_the_gpu():
    x = [torch.zeros(5, 64)]  # CPU tensors: a call in order would be refused as such, last of all
    with pytest.raises(ValueError, match="mode='global' only"):
        esm_amd.align_embeddings(x, x, mode="local", free_ends="b")
    with pytest.raises(ValueError, match="mode.*free_ends="):
        esm_amd.align_embeddings(x, x, mode="semiglobal")
    with pytest.raises(ValueError, match="free_ends"):
        esm_amd.align_embeddings(x, x, free_ends=16)
    for k in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="hits_per_pair must be"):
            esm_amd.align_embeddings(x, x, mode="local", hits_per_pair=k)
    with pytest.raises(ValueError, match="needs paths=True"):
        esm_amd.align_embeddings(x, x, hits_per_pair=2, paths=False)
    with pytest.raises(ValueError, match="return_similarity"):
        esm_amd.align_embeddings(x, x, hits_per_pair=2, return_similarity=True)
    with pytest.raises(ValueError, match="NaN"):
        esm_amd.align_embeddings(x, x, hits_per_pair=2, min_hit_score=float("nan"))
    for kw in (dict(free_ends="both"), dict(mode="local", hits_per_pair=3), dict(free_ends=["a_end"], hits_per_pair=16)):
        with pytest.raises(RuntimeError, match="MI355X"):  # in order: only the device is missing
            esm_amd.align_embeddings(x, x, **kw)


def test_model_and_search_refusals():
    model = esm.ESM2(2, 64, 2).eval()
    toks = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="mode='global' only"):
        model.align(toks, toks, mode="local", free_ends="a")
    with pytest.raises(ValueError, match="hits_per_pair must be"):
        model.align(toks, toks, hits_per_pair=0)
    with pytest.raises(ValueError, match="needs paths=True"):
        model.align(toks, toks, hits_per_pair=2, paths=False)

    class Index:
        sequences = ["MKV"]

    depth, *_, kw = MB.check_args(Index(), align_kw=dict(mode="global", free_ends="b", hits_per_pair=3, min_hit_score=1.0))
    assert kw == dict(mode="global", enhance=True, free_ends="b", hits_per_pair=3, min_hit_score=1.0)
    assert MB.check_args(Index())[5] == dict(mode="local", enhance=True)  # the defaults are what they were
    assert MB.check_args(Index(), align_kw=dict(hits_per_pair=2))[5]["mode"] == "local"
    with pytest.raises(ValueError, match="mode='global' only"):
        MB.check_args(Index(), align_kw=dict(free_ends="b"))  # the module's default mode is local
    with pytest.raises(ValueError, match="hits_per_pair must be"):
        MB.check_args(Index(), align_kw=dict(hits_per_pair=17))


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_ex_entries_refuse_before_any_hip_call():
    L, null, p = N.lib, None, 4096  # p: a non-null, aligned address that is never dereferenced
    dp = lambda **k: L.esmk_op_align_dp_ex(*[k.get(n, d) for n, d in (
        ("S", p), ("ld", 64), ("rows", 8), ("cols", 64), ("table", p), ("n", 1), ("mode", 0), ("fe", 0), ("o", 1.0), ("e", 0.1), ("la", 8),
        ("lb", 8), ("score", p), ("end", p), ("tb", p), ("tbn", 1024), ("want", 1), ("ws", null), ("wsn", 0), ("stream", null))])
    for bad in (dict(fe=16), dict(fe=-1), dict(fe=1, mode=1), dict(fe=15, mode=1), dict(mode=2), dict(e=2.0), dict(S=p + 4), dict(tb=null)):
        assert dp(**bad) != 0, bad
        assert "esmk_op_align_dp_ex" in L.esmk_last_error().decode()
    assert "free_ends" in (dp(fe=16), L.esmk_last_error().decode())[1]
    assert dp(n=0) == 0 and dp(n=0, fe=15) == 0  # nothing to do: nothing is launched
    tr = lambda **k: L.esmk_op_align_traceback_ex(*[k.get(n, d) for n, d in (
        ("table", p), ("n", 1), ("mode", 0), ("fe", 0), ("end", p), ("tb", p), ("tbn", 64), ("slot", p), ("cols", p), ("cap", 16),
        ("ncols", p), ("nmatch", p), ("start", p), ("S", null), ("ld", 0), ("rows", 0), ("scols", 0), ("stream", null))])
    good = dict(S=p, ld=64, rows=8, scols=64)
    for bad in (dict(fe=16), dict(fe=-1), dict(fe=4, mode=1), dict(mode=3), dict(tb=null),
                dict(ld=64, rows=8, scols=64),            # dimensions without a mask
                dict(good, S=p + 4),                      # misaligned
                dict(good, scols=60), dict(good, ld=60), dict(good, rows=0), dict(good, ld=66)):
        assert tr(**bad) != 0, bad
        assert "esmk_op_align_traceback_ex" in L.esmk_last_error().decode()
    assert tr(n=0) == 0 and tr(n=0, fe=12, **good) == 0
    # the plain entries forward with free_ends = 0: their refusals and names are what they were
    assert L.esmk_op_align_dp(p, 64, 8, 64, p, 1, 2, 1.0, 0.1, 8, 8, p, p, p, 1024, 1, null, 0, null) != 0
    assert "esmk_op_align_dp: mode must be 0 (global) or 1 (local)" in L.esmk_last_error().decode()
    assert L.esmk_op_align_traceback(p, 1, 2, p, p, 64, p, p, 16, p, p, p, null) != 0
    assert "esmk_op_align_traceback: mode must be" in L.esmk_last_error().decode()


# ---- command lines ------------------------------------------------------------------------------------------------------
def test_command_line_options():
    base = ["--model-location", "m.pt", "--query", "q.fa", "--target", "t.fa", "--output", "hits.tsv"]
    a = A.parse_args(base)
    assert (a.mode, a.free_ends, a.hits_per_target) == ("global", None, 1)
    a = A.parse_args(base + ["--free-ends", "b", "--hits-per-target", "3", "--top", "5"])
    assert (a.mode, a.free_ends, a.hits_per_target, a.top) == ("global", "b", 3, 5)
    assert A.parse_args(base + ["--free-ends", "both", "--mode", "global"]).mode == "global"
    assert A.parse_args(base + ["--mode", "local", "--hits-per-target", "2"]).mode == "local"
    for bad in (["--free-ends", "b", "--mode", "local"], ["--free-ends", "c"], ["--hits-per-target", "0"], ["--hits-per-target", "17"]):
        with pytest.raises(SystemExit):
            A.parse_args(base + bad)
    q = ["query", "--model-location", "m.pt", "--index", "db.npz", "--query", "q.fa", "--top", "5", "--output", "o.tsv"]
    s = SE.parse_args(q + ["--align", "--free-ends", "b", "--hits-per-target", "2"])
    assert (s.mode, s.free_ends, s.hits_per_target) == ("global", "b", 2)
    assert SE.parse_args(q).mode == "global" and SE.parse_args(q + ["--align", "--mode", "local"]).mode == "local"
    for bad in (["--free-ends", "b"], ["--hits-per-target", "2"], ["--align", "--free-ends", "a", "--mode", "local"]):
        with pytest.raises(SystemExit):
            SE.parse_args(q + bad)
    m = ["--model-location", "m.pt", "--index", "db.npz", "--query", "q.fa", "--output-dir", "out"]
    b = MB.parse_args(m)
    assert (b.mode, b.free_ends, b.hits_per_target) == ("local", None, 1)
    b = MB.parse_args(m + ["--free-ends", "b", "--hits-per-target", "4"])
    assert (b.mode, b.free_ends, b.hits_per_target) == ("global", "b", 4)
    with pytest.raises(SystemExit):
        MB.parse_args(m + ["--free-ends", "b", "--mode", "local"])


def test_tsv_gains_a_hit_column_only_on_request():
    hits = [dict(query="q1", target="t1", score=3.25, la=4, lb=8, n_match=3, start=[1, 0], end=[4, 3], hit=0),
            dict(query="q1", target="t1", score=2.0, la=4, lb=8, n_match=2, start=[0, 5], end=[2, 7], hit=1)]
    fh = io.StringIO()
    A.write_tsv(fh, hits)
    assert fh.getvalue().splitlines()[0].split("\t") == list(A.TSV_HEADER) and len(fh.getvalue().splitlines()[1].split("\t")) == 7
    fh = io.StringIO()
    A.write_tsv(fh, hits, hit_column=True)
    lines = [line.split("\t") for line in fh.getvalue().splitlines()]
    assert lines[0] == list(A.TSV_HEADER) + ["hit"] and lines[1][-1] == "0" and lines[2] == ["q1", "t1", "2.0000", "0.5000", "2", "1-2", "6-7", "1"]
    fh = io.StringIO()
    SE.write_tsv(fh, [dict(h, rank=1, cosine=0.5) for h in hits], aligned=True, hit_column=True)
    lines = [line.split("\t") for line in fh.getvalue().splitlines()]
    assert lines[0] == list(SE.TSV_HEADER) + list(A.TSV_HEADER[2:]) + ["hit"] and lines[2][-1] == "1"
